"""The decimator's committed tables (csrc/tl_decimate_taps.inc): a fresh run of the generator gives the committed text, the shapes and row
sums, the quarter bound the kernel's 32-bit partial sums rest on, and the frequency response computed from the table alone."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import decimatelib as D

ROOT = Path(__file__).resolve().parent.parent
PAIRS = [(48000, 1, 2), (32000, 3, 4), (44100, 80, 147)]


def test_committed_table_is_the_generator_s():
    spec = importlib.util.spec_from_file_location("gen_decimate_taps", ROOT / "tools" / "gen_decimate_taps.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.text() == (ROOT / "odr-audioenc_amd" / "csrc" / "tl_decimate_taps.inc").read_text()


@pytest.mark.parametrize("source,L,M", PAIRS)
def test_shapes_sums_and_the_quarter_bound(source, L, M):
    H = D.taps(source, 24000)
    assert H.shape == (L, 64)
    assert (H.sum(axis=1) == 32768).all()
    quarters = np.abs(H).reshape(L, 4, 16).sum(axis=2)
    print(source, "largest quarter", quarters.max(), "largest row", np.abs(H).sum(axis=1).max())
    assert quarters.max() < 65536                                    # a quarter times 32768 stays below 2^31
    assert quarters.max() <= 40811                                   # ... the figure csrc/mp2_decimate.h states


@pytest.mark.parametrize("source,L,M", PAIRS)
def test_response_from_the_table_alone(source, L, M):
    """h[p + L t] = H[p][t] is the prototype at L x the source rate, gain L * 32768; the output's Nyquist frequency is 0.5 / M cycles per
    sample there.  Passband within +- 0.05 dB up to 0.8 x of it, at least 70 dB down from 1.2 x upwards (the recipe gives a ripple of at most
    0.009 dB and - 75.7 / - 78.6 / - 85.7 dB for 1/2, 3/4, 80/147: the margin is ours, the reference has nothing to compare with)."""
    H = D.taps(source, 24000)
    h = np.zeros(L * 64)
    for p in range(L):
        h[p::L] = H[p]
    nfft = 1 << 20
    F = np.abs(np.fft.rfft(h, nfft)) / (L * 32768.0)
    f = np.arange(len(F)) / nfft
    ny = 0.5 / M
    pb = 20 * np.log10(F[f <= 0.8 * ny])
    sb = 20 * np.log10(F[f >= 1.2 * ny].max())
    print(source, "passband %.4f .. %.4f dB, stopband %.1f dB" % (pb.min(), pb.max(), sb))
    assert pb.min() >= -0.05 and pb.max() <= 0.05
    assert sb <= -70.0
