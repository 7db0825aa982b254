"""The decimator's kernel text as lane loops (tests/emu/mp2_decimate_emu.cpp) against the oracle (tests/decimatelib.py: the header's
formula over numpy int64), byte for byte: the shared six streams over six frames, cut three ways."""
import subprocess

import numpy as np
import pytest

import decimatelib as D

S = D.STREAMS
DOWN = [s for s, c in enumerate(S) if c["source"]]


@pytest.fixture(scope="module")
def noise():
    sigs = D.signals(S, "noise")
    bg = D.background(D.NFRAMES, len(S))
    return sigs, bg, D.Oracle(S).decimate(D.cut(sigs, S, 0, D.NFRAMES), bg)


@pytest.mark.parametrize("cuts", D.CUTS)
def test_noise_equals_oracle_however_cut(noise, cuts):
    sigs, bg, want = noise
    assert sum(cuts) == D.NFRAMES
    got = D.run_cuts(D.DecimateEmu(S).decimate, sigs, S, cuts, bg=bg)
    assert np.array_equal(got, want), (cuts, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("cuts", D.CUTS)
def test_full_scale_square_exercises_the_clamp(cuts):
    sigs = D.signals(S, "square")
    for s in DOWN:                                                   # on the oracle's UNCLAMPED sums: both sides leave the int16 range
        y = (D.oracle_stream(sigs[s], S[s]["source"], 24000, D.N, unclamped=True) + 16384) >> 15
        assert y.max() > 32767 and y.min() < -32768, (s, y.max(), y.min())
    want = D.Oracle(S).decimate(D.cut(sigs, S, 0, D.NFRAMES))
    assert want.max() == 32767 and want.min() == -32768
    got = D.run_cuts(D.DecimateEmu(S).decimate, sigs, S, cuts)
    assert np.array_equal(got, want), cuts


@pytest.mark.parametrize("c", [32767, -32768])
def test_constant_in_constant_out(c):
    """every row sums to 32768: from output 64 on all 64 taps lie on the input (q(64) >= 63 for every ratio) and the output is exactly c"""
    sigs = D.signals(S, ("const", c), 2)
    got = D.DecimateEmu(S).decimate(D.cut(sigs, S, 0, 2))
    assert np.array_equal(got, D.Oracle(S).decimate(D.cut(sigs, S, 0, 2)))
    for s in DOWN:
        nch = D.nch_of(S[s])
        y = got[:, s, :nch * D.N].reshape(-1, nch)
        assert (y[64:] == c).all() and not (y[:64] == c).all(), s


@pytest.mark.parametrize("source", [48000, 32000, 44100])
def test_adversarial_source_reaches_the_quarter_bound(source):
    """the input that drives every tap of the row with the largest quarter to full scale with the tap's sign: each 16-tap quarter reaches
    sum |H| * 32768 in 32 bits (it fits), the whole row does not -- a 32-bit whole-row sum wraps and comes out with the wrong sign.  The
    64-bit oracle says what the answer is."""
    x, n, p = D.adversarial(source, 24000)
    H = D.taps(source, 24000)
    acc = D.oracle_stream(x, source, 24000, 1, n0=n, unclamped=True)[0, 0]
    pos, neg = int(H[p][H[p] > 0].sum()), int(-H[p][H[p] < 0].sum())
    assert acc == -(32768 * pos + 32767 * neg)                       # every tap pulls the same way
    if source == 32000:                                              # sum |H[p]| = 67 496: the exact sum is outside 32 bits (1/2 and 80/147 stay just inside)
        assert abs(acc) >= 2 ** 31, acc
    assert np.abs(H[p]).reshape(4, 16).sum(axis=1).max() * 32768 < 2 ** 31
    cfgs = [dict(samplerate=24000, mode="m", source=source), dict(samplerate=24000, mode="s", source=source)]
    nf = n // D.N + 1
    sigs = []
    for c in cfgs:
        v = np.zeros((D.total_need(c, nf), D.nch_of(c)), dtype=np.int16)
        v[:len(x)] = x                                               # (both channels of the two-channel stream)
        sigs.append(v)
    wide = D.cut(sigs, cfgs, 0, nf)
    want = D.Oracle(cfgs).decimate(wide)
    assert want[n // D.N, 0, n % D.N] == -32768 and want[n // D.N, 1, 2 * (n % D.N) + 1] == -32768
    got = D.DecimateEmu(cfgs).decimate(wide)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


def test_nothing_else_is_read_or_written(noise):
    """0x7FFF in every value behind the need frames and in the whole wide slot of streams 4 and 5: the outputs do not change, the output slots
    of streams 4 and 5 and the second half of a one-channel slot keep what they held"""
    sigs, bg, want = noise
    got = D.run_cuts(D.DecimateEmu(S).decimate, sigs, S, (1, 3, 2), fill=0x7FFF, bg=bg)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 4:], bg[:, 4:])
    for s in (1, 3):
        assert np.array_equal(got[:, s, D.N:], bg[:, s, D.N:]) and not np.array_equal(got[:, s, :D.N], bg[:, s, :D.N])


def test_reset_in_the_middle(noise):
    sigs, bg, want = noise
    e, o = D.DecimateEmu(S), D.Oracle(S)
    first = D.cut(sigs, S, 0, 3)
    assert np.array_equal(e.decimate(first), o.decimate(first))
    e.reset(2); o.reset(2)
    nxt = D.cut(sigs, S, 3, 2)
    nxt[:, 2] = D.cut(sigs, S, 0, 2)[:, 2]                           # stream 2 (80/147) starts again: need(0), need(1) frames of its source
    got = e.decimate(nxt, bg[:2].copy())
    assert np.array_equal(got, o.decimate(nxt, bg[:2]))
    assert np.array_equal(got[:, 2], want[:2, 2])                    # ... and gives what a fresh stream gave
    for s in (0, 1, 3):
        nch = D.nch_of(S[s])
        assert np.array_equal(got[:, s, :nch * D.N], want[3:5, s, :nch * D.N])      # the others go on


def test_sanitized_stand_alone_driver():
    """the same emulation text behind a main of its own, built with AddressSanitizer + UBSan and run as a program (nothing preloaded): the LDS
    layouts, the table rows and the slots stay inside their arrays, and the three cuts agree"""
    r = subprocess.run([str(D.build_sanitized())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sanitized ok" in r.stdout and not r.stderr.strip(), (r.returncode, r.stdout, r.stderr[-2000:])
