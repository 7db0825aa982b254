"""The resampler's kernel text as lane loops (tests/emu/mp2_resample_emu.cpp) against the oracle (tests/resamplelib.py: the header's two
formulas over numpy int64), byte for byte: the issue's five streams over six frames, cut three ways."""
import numpy as np
import pytest

import resamplelib as R

S = R.STREAMS


@pytest.fixture(scope="module")
def noise():
    sigs = R.signals(S, "noise")
    return sigs, R.Oracle(S).resample(R.cut(sigs, S, 0, R.NFRAMES))


@pytest.mark.parametrize("cuts", R.CUTS)
def test_noise_equals_oracle_however_cut(noise, cuts):
    sigs, want = noise
    got = R.run_cuts(R.ResampleEmu(S).resample, sigs, S, cuts)
    assert sum(cuts) == R.NFRAMES
    R.same(got, want, S, cuts)
    assert np.array_equal(got[:, 4], R.cut(sigs, S, 0, R.NFRAMES)[:, 4])      # the stream without a source: its slot as it is


@pytest.mark.parametrize("cuts", R.CUTS)
def test_full_scale_square_exercises_the_clamp(cuts):
    sigs = R.signals(S, "square")
    for s, c in enumerate(S[:4]):                                    # on the oracle's UNCLAMPED sums: both sides leave the int16 range
        acc = R.oracle_stream(sigs[s], c["source"], c["samplerate"], R.N, unclamped=True)
        y = (acc + 16384) >> 15
        assert y.max() > 32767 and y.min() < -32768, (s, y.max(), y.min())
    want = R.Oracle(S).resample(R.cut(sigs, S, 0, R.NFRAMES))
    assert want.max() == 32767 and want.min() == -32768
    R.same(R.run_cuts(R.ResampleEmu(S).resample, sigs, S, cuts), want, S, cuts)


@pytest.mark.parametrize("c", [-32768, -1, 12345, 32767])
def test_constant_in_constant_out(c):
    """every row sums to 32768: once all 32 taps lie on the input (q(n) >= 31) the output is exactly c"""
    sigs = R.signals(S, ("const", c), 2)
    got = R.ResampleEmu(S).resample(R.cut(sigs, S, 0, 2))
    R.same(got, R.Oracle(S).resample(R.cut(sigs, S, 0, 2)), S)
    for s, cfg in enumerate(S[:4]):
        L, M = R.ratio_of(cfg["source"], cfg["samplerate"])
        n0 = -(-(R.T - 1) * L // M)                                  # the first n with q(n) >= T - 1
        assert R.q_of(n0, L, M) >= R.T - 1 > R.q_of(n0 - 1, L, M)
        nch = R.nch_of(cfg)
        y = got[:, s, :nch * R.N].reshape(-1, nch)
        assert (y[n0:] == c).all() and not (y[:n0] == c).all(), s


def test_sine_against_the_least_squares_sine():
    """997 Hz at amplitude 16000: the output against the least-squares sine of that frequency at the encoder's rate; the ratio of signal to
    residual is at least 75 dB for both ratios (the first frame, which holds the start-up, is left out)"""
    sigs = R.signals(S, ("sine", 997.0, 16000.0))
    got = R.ResampleEmu(S).resample(R.cut(sigs, S, 0, R.NFRAMES))
    for s, cfg in enumerate(S[:4]):
        nch = R.nch_of(cfg)
        y = got[1:, s, :nch * R.N].reshape(-1, nch)[:, 0].astype(np.float64)
        k = np.arange(len(y), dtype=np.float64)
        A = np.stack([np.sin(2 * np.pi * 997.0 * k / cfg["samplerate"]), np.cos(2 * np.pi * 997.0 * k / cfg["samplerate"])], axis=1)
        coef, *_ = np.linalg.lstsq(A, y, rcond=None)
        res = y - A @ coef
        snr = 10 * np.log10((A @ coef).dot(A @ coef) / res.dot(res))
        print("stream", s, "signal / residual %.1f dB, amplitude %.1f" % (snr, np.hypot(*coef)))
        assert snr >= 75.0, (s, snr)
        assert abs(np.hypot(*coef) - 16000.0) < 16.0


def test_values_behind_need_are_never_read(noise):
    sigs, want = noise
    got = R.run_cuts(R.ResampleEmu(S).resample, sigs, S, (1, 3, 2), fill=0x7FFF)
    R.same(got[:, :4], want[:, :4], S[:4])


def test_reset_in_the_middle(noise):
    sigs, want = noise
    e, o = R.ResampleEmu(S), R.Oracle(S)
    first = R.cut(sigs, S, 0, 3)
    R.same(e.resample(first), o.resample(first), S)
    e.reset(0); o.reset(0)                                           # (that the library's need is need(0) again is the GPU life-cycle test's: the emulation has no need of its own)
    nxt = R.cut(sigs, S, 3, 2)
    nxt[:, 0] = R.cut(sigs, S, 0, 2)[:, 0]                           # stream 0 starts again: need(0), need(1) frames of its source
    got = e.resample(nxt)
    R.same(got, o.resample(nxt), S)
    assert np.array_equal(got[:, 0], want[:2, 0])                    # ... and gives what a fresh stream gave
    R.same(got[:, 1:], want[3:5, 1:], S[1:])                         # the others go on
