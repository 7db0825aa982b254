"""The committed polyphase tables of the device resampler (csrc/tl_resample_taps.inc through tlb_resample_taps): row sums, range, the
response computed from the table itself, the bound the kernel's 32-bit partial sums rest on, and the generating tool's recipe."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import resamplelib as R

ROOT = Path(__file__).resolve().parent.parent
PAIRS = [(44100, 48000), (32000, 48000)]


@pytest.mark.parametrize("pair", PAIRS)
def test_rows_sum_to_unity_and_fit_int16(pair):
    import odr_audioenc_amd as M
    H, L, Mm = M.resample_taps(*pair)
    assert H.dtype == np.int16 and H.shape == (L, 32) and (L, Mm) == R.ratio_of(*pair)
    H = H.astype(np.int64)
    assert (H.sum(axis=1) == 32768).all()
    assert H.min() >= -32768 and H.max() <= 32767
    assert int(np.abs(H).sum(axis=1).max()) == {160: 71674, 3: 71568}[L]      # a whole row does not fit 32 bits: 71 674 * 32 768 > 2^31


def test_the_two_rates_of_a_ratio_share_one_table():
    import odr_audioenc_amd as M
    for a, b in (((44100, 48000), (22050, 24000)), ((32000, 48000), (16000, 24000))):
        assert np.array_equal(M.resample_taps(*a)[0], M.resample_taps(*b)[0])
    for pair in ((48000, 24000), (48000, 44100), (44100, 24000), (48000, 48000), (0, 48000)):
        assert M.resample_taps(*pair) is None


@pytest.mark.parametrize("pair", PAIRS)
def test_response_of_the_table(pair):
    """The prototype at L x the source rate, read back from the table: h[k] = H[k % L][k // L] / 32768.  Pass band 0 .. 0.8 x the source's
    Nyquist frequency within +- 0.02 dB of unity (gain L over the zero-stuffed input); the images of that band, from source rate - 0.8 x
    Nyquist upward, at or below - 75 dB."""
    H = R.taps(*pair).astype(np.float64)
    L = H.shape[0]
    h = (H.T.reshape(-1)) / 32768.0                                   # k = t * L + p
    nfft = 1 << 20
    mag = np.abs(np.fft.rfft(h, nfft))
    f = np.arange(len(mag)) / nfft                                    # cycles per sample at L x source rate; the source's Nyquist is 0.5 / L
    nyq = 0.5 / L
    pb = mag[f <= 0.8 * nyq] / L                                      # rows sum to 1, so h sums to L: unity is |H(f)| = L
    db = 20 * np.log10(pb)
    print(pair, "pass band %.4f .. %.4f dB" % (db.min(), db.max()))
    assert db.min() >= -0.02 and db.max() <= 0.02
    sb = mag[f >= 2 * nyq - 0.8 * nyq] / L
    sdb = 20 * np.log10(sb.max())
    print(pair, "images %.1f dB" % sdb)
    assert sdb <= -75.0


@pytest.mark.parametrize("pair", PAIRS)
def test_half_rows_cannot_overflow_32_bits(pair):
    """csrc/mp2_resample.h sums taps 0..15 and 16..31 of a row in 32 bits each: |x| <= 32768, so sum |H| * 32768 must stay below 2^31"""
    H = np.abs(R.taps(*pair))
    for half in (H[:, :16], H[:, 16:]):
        assert int(half.sum(axis=1).max()) * 32768 < 2 ** 31
    assert int(H.sum(axis=1).max()) * 32768 >= 2 ** 31                # ... which a whole row would not


def test_tool_follows_the_recipe_of_the_committed_file(tmp_path):
    """The committed table is the definition whatever the tool gives; the tool is the record of the recipe.  Its doubles come from numpy's
    kaiser / i0 / sinc and the platform's libm, so a tap that lies within an ulp of .5 before rounding may land on the other side elsewhere:
    the tool's table must have the committed shape, rows summing to 32768, and no tap further than 1 from the committed one."""
    import re
    out = tmp_path / "taps.inc"
    subprocess.run([sys.executable, str(ROOT / "tools" / "gen_resample_taps.py"), str(out)], check=True, capture_output=True)
    text = out.read_text()
    for pair in PAIRS:
        H = R.taps(*pair)
        L, Mm = R.ratio_of(*pair)
        m = re.search(r"tl_resample_taps_%d_%d\[%d\]\[32\] = \{(.*?)\n\};" % (L, Mm, L), text, re.S)
        assert m, pair
        G = np.array([int(v) for v in re.findall(r"-?\d+", m.group(1))], dtype=np.int64).reshape(L, 32)
        assert (G.sum(axis=1) == 32768).all() and int(np.abs(G - H).max()) <= 1, pair
