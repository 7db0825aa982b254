"""The limiter's kernel as lane loops (tests/emu/mp2_limiter_emu.cpp: csrc/mp2_limiter.h with -DTL_EMULATE) against the definition restated
in numpy int64 (limiterlib.Oracle), byte for byte on the PCM and on the records: the 37-stream set in three cuts, the constructed cases, both
paths and both transitions between them, the life-cycle calls in mid-run; the theorem (32768 |y| <= ceiling) on every case and on 300
random signals; the output's true peak, measured with the true-peak meter's oracle at the same ceiling: no over on the structured
signals, and on the random ones an excess below the 0.2 dB that tests/test_truepeak_emu.py grants the meter itself (measured here with the
oracle: at most 0.00071 dB, 88 292 units of 2^-30); and the same emulation as a program of its own under AddressSanitizer + UBSan."""
import subprocess

import numpy as np
import pytest

import limiterlib as LM
import truepeaklib as TP

N, U = LM.N, LM.U


def _check(got, want, what):
    (gp, gr), (wp, wr) = got, want
    bad = [s for s in range(len(wr)) if not np.array_equal(gp[:, s], wp[:, s]) or gr[s].tobytes() != wr[s].tobytes()]
    assert not bad, (what, bad[:6], gr[bad[0]], wr[bad[0]])


def _mono(x):
    return [dict(samplerate=48000, mode="m")], LM.one_stream(x)


@pytest.fixture(scope="module")
def pcm():
    return LM.pcm_of(LM.STREAMS)


@pytest.fixture(scope="module")
def oracle(pcm):
    """the oracle's PCM and its records after every frame count at which some cut ends: computed once"""
    o = LM.Oracle(LM.STREAMS)
    ends = sorted({sum(c[:i + 1]) for c in LM.CUTS[0:1] + LM.CUTS[2:] for i in range(len(c))})
    out, recs, f0 = [], {}, 0
    for e in ends:
        p, recs[e] = o.limit(pcm[f0:e])
        out.append(p)
        f0 = e
    return np.concatenate(out), recs


def test_the_closed_form_of_the_release_is_the_recurrence():
    rng = np.random.default_rng(1)
    m = np.where(rng.random(3000) < 0.01, rng.integers(1 << 20, 1 << 30, 3000), U).astype(np.int64)
    k = np.arange(3000, dtype=np.int64)
    for S in (1, 223696, 1 << 26):
        e = np.minimum(U, np.minimum(np.minimum.accumulate(m - k * S) + k * S, 12345678 + (k + 1) * S))
        assert np.array_equal(e, LM.release_serial(m, S, 12345678))


def test_oracle_sees_every_part_of_the_definition(pcm, oracle):
    out, recs = oracle
    r = recs[LM.NFRAMES]
    assert len(LM.STREAMS) == 37 and (r["frames"] == LM.NFRAMES).all() and not r["reserved"].any()
    kinds = [LM.LL.KINDS[s % 7] for s in range(37)]
    loud = [s for s in range(37) if kinds[s] in (("noise", 0.0), ("square", 0.0))]
    quiet = [s for s in range(37) if kinds[s][0] == "silence" or kinds[s] in (("noise", -20.0), ("noise", -45.0), ("noise", -80.0))]
    assert (r["limited"][loud] == LM.NFRAMES).all() and r["red_max"][loud].all() and (r["peak_in_max"][loud] > LM.CEILING_DEFAULT).all()
    assert not r["limited"][quiet].any() and not r["samples"][quiet].any() and not r["red_max"][quiet].any()
    for s in quiet:                                                  # at or below the ceiling: the input itself, 63 samples late
        for c in range(LM.nch_of(LM.STREAMS[s])):
            x, y = pcm[:, s, c].reshape(-1), out[:, s, c].reshape(-1)
            assert np.array_equal(y[63:], x[:-63]) and not y[:63].any(), s
    mono = [s for s in range(37) if LM.nch_of(LM.STREAMS[s]) == 1]
    assert np.array_equal(out[:, mono, 1], pcm[:, mono, 1])          # a one-channel stream's second row comes back as it went in
    assert (32768 * np.abs(out.astype(np.int64)[:, :, 0]) <= LM.CEILING_DEFAULT).all()


@pytest.mark.parametrize("cuts", LM.CUTS, ids=["one", "frames", "7+38"])
def test_emulation_equals_the_definition(pcm, oracle, cuts):
    out, recs = oracle
    e = LM.LimiterEmu(LM.STREAMS)
    p0 = e.path_counts()
    f0 = 0
    for n in cuts:
        gp, gr = e.limit(pcm[f0:f0 + n])
        assert np.array_equal(gp, out[f0:f0 + n]), (f0, [s for s in range(37) if not np.array_equal(gp[:, s], out[f0:f0 + n, s])][:6])
        f0 += n
        if f0 in recs:
            assert LM.same(gr, recs[f0]), (f0, [s for s in range(37) if gr[s].tobytes() != recs[f0][s].tobytes()][:6])
    assert LM.same(e.rec, recs[LM.NFRAMES])
    p1 = e.path_counts()
    assert p1[0] > p0[0] and p1[1] > p0[1] and (p1[0] - p0[0]) + (p1[1] - p0[1]) == 37 * LM.NFRAMES      # both paths ran


@pytest.mark.parametrize("cuts", [(4,), (1, 1, 1, 1), (2, 2)], ids=["one", "frames", "2+2"])
@pytest.mark.parametrize("ceiling,ms", [(0, 0), (300000000, 1), (1 << 20, 5), (1 << 30, 10000)], ids=["default", "300M 1ms", "2^20 5ms", "2^30 10s"])
def test_constructed_cases(cuts, ceiling, ms):
    cfgs, x, names = LM.constructed()
    o, e = LM.Oracle(cfgs, ceiling, ms), LM.LimiterEmu(cfgs, ceiling, ms)
    f0, outs = 0, []
    for n in cuts:
        want, got = o.limit(x[f0:f0 + n]), e.limit(x[f0:f0 + n])
        _check(got, want, (cuts, f0))
        outs.append(want[0]); f0 += n
    y, r = np.concatenate(outs), o.rec
    lim = ceiling if ceiling else LM.CEILING_DEFAULT
    for s, c in enumerate(cfgs):                                     # the theorem, on the rows the stream has; a one-channel stream's second row is untouched
        assert (32768 * np.abs(y[:, s, :LM.nch_of(c)].astype(np.int64)) <= lim).all(), names[s]
        assert LM.nch_of(c) == 2 or np.array_equal(y[:, s, 1], x[:, s, 1]), names[s]
    assert (y[:, 0, 1] == 0x5a5a).all()                              # the poisoned second row of the mono stream
    if ceiling == 0:
        # the over at n = 0 of frame 1 leaves at n = 63 of frame 1, the one at n = 1151 at n = 62 of frame 2, both at the ceiling
        assert abs(int(y[1, 0, 0, 63])) > 29000 and abs(int(y[2, 0, 0, 62])) > 29000
        assert r["limited"][0] >= 2 and r["peak_in_max"][0] == 2 ** 30
        # an over in channel 1 only: channel 0 drops as well, by the same gain
        flat0, in0 = y[:, 1, 0].reshape(-1), x[:, 1, 0].reshape(-1).astype(np.int64)
        at = 1 * N + 600 + 63                                        # where the over leaves
        assert abs(int(flat0[at])) < abs(int(in0[at - 63])) and r["limited"][1] >= 1
        assert r["limited"][4] == 2 and r["red_max"][4] > 0            # the over at n = 1000 leaves at 1063 and its release (about 350 samples) ends in frame 1
        # the quiet stream is never touched
        assert not r["limited"][5] and np.array_equal(y[:, 5].transpose(1, 0, 2).reshape(2, -1)[:, 63:], x[:, 5].transpose(1, 0, 2).reshape(2, -1)[:, :-63])


def test_a_release_over_three_frames_and_two_calls():
    """32 kHz mono, ceiling 2^20, one full-scale sample at n = 1000 of frame 0 in silence: the gain falls to 2^20 / 2^30 and recovers over
    100 ms = 3200 samples, through frames 1, 2 and into 3, across the boundary between two calls"""
    cfgs = [dict(samplerate=32000, mode="m")]
    x = np.zeros((4, 1, 2, N), dtype=np.int16); x[0, 0, 0, 1000] = 32767
    o, e = LM.Oracle(cfgs, 1 << 20, 100), LM.LimiterEmu(cfgs, 1 << 20, 100)
    _check(e.limit(x[:2]), o.limit(x[:2]), "first call")
    mid = o.rec.copy()
    _check(e.limit(x[2:]), o.limit(x[2:]), "second call")
    r = o.rec
    assert mid["limited"][0] == 2 and r["limited"][0] == 4 and 0 < r["red_last"][0] < mid["red_last"][0] <= r["red_max"][0] == 65536 - 64
    assert 1152 + 2 * 1152 < 1000 + 63 + 3200 < 4 * 1152 and r["samples"][0] < 4 * N


def test_minus_32768_at_unity_gain():
    """ceiling 2^30: a lone -32768 has P = 2^30 exactly (every |H| is below 32768), which is not over: it comes out as itself"""
    x = np.zeros(2 * N, dtype=np.int16); x[100] = -32768; x[N - 1] = -32768; x[N + 200] = 32767      # far enough apart that no interpolation sees two of them
    cfgs, p = _mono(x)
    o, e = LM.Oracle(cfgs, 1 << 30), LM.LimiterEmu(cfgs, 1 << 30)
    want, got = o.limit(p), e.limit(p)
    _check(got, want, "unity")
    y = want[0][:, 0, 0].reshape(-1)
    assert y[163] == -32768 and y[N + 62] == -32768 and y[N + 263] == 32767 and np.count_nonzero(y) == 3 and not want[1]["limited"][0] and want[1]["peak_in_max"][0] == 2 ** 30


def test_idle_to_active_to_idle_and_a_reset_in_the_middle():
    """the 24 kHz stream with a 5 ms release (120 samples), frame by frame: idle, active (the over), then idle again once the carried gains
    are back at unity; after a reset in mid-release the next frame starts from unity"""
    cfgs, x, _ = LM.constructed()
    cfgs, x = cfgs[3:4], x[:, 3:4]
    o, e = LM.Oracle(cfgs, 0, 5), LM.LimiterEmu(cfgs, 0, 5)
    paths = []
    for f in range(4):
        p0 = e.path_counts()
        _check(e.limit(x[f:f + 1]), o.limit(x[f:f + 1]), f)
        p1 = e.path_counts()
        paths.append((p1[0] - p0[0], p1[1] - p0[1]))
    assert paths == [(1, 0), (0, 1), (1, 0), (1, 0)], paths
    assert o.rec["limited"][0] == 1 and o.rec["red_last"][0] == 0 and o.rec["red_max"][0] > 0
    # a long release: still active when the reset comes
    o, e = LM.Oracle(cfgs, 0, 1000), LM.LimiterEmu(cfgs, 0, 1000)
    _check(e.limit(x[:2]), o.limit(x[:2]), "before")
    assert o.rec["red_last"][0] > 0
    o.reset(0); e.reset(0)
    p0 = e.path_counts()
    want = o.limit(x[2:3])
    _check(e.limit(x[2:3]), want, "after")
    assert e.path_counts()[0] == p0[0] + 1 and want[1]["frames"][0] == 1 and not want[1]["limited"][0] and not want[0][0, 0, :, :63].any()


def test_reset_and_reconfigure_in_mid_run(pcm):
    """after 12 frames: stream 3 is reset, stream 8 (32 kHz stereo) becomes 16 kHz mono (another S, one channel), all go on for 6 frames"""
    new = dict(samplerate=16000, mode="m")
    o, e = LM.Oracle(LM.STREAMS), LM.LimiterEmu(LM.STREAMS)
    _check(e.limit(pcm[:12]), o.limit(pcm[:12]), "first")
    for x in (o, e):
        x.reset(3)
        x.reconfigure(8, new)
    want = o.limit(pcm[12:18])
    _check(e.limit(pcm[12:18]), want, "second")
    assert want[1]["frames"][3] == 6 and want[1]["frames"][8] == 6 and want[1]["frames"][4] == 18
    assert np.array_equal(want[0][:, 8, 1], pcm[12:18, 8, 1])


@pytest.fixture(scope="module")
def randoms():
    return LM.random_signals()


def test_the_theorem_and_the_true_peak_on_300_random_signals(randoms):
    """per signal: emulation = oracle; 32768 |y| <= ceiling; the output's true peak by the meter's oracle at the same ceiling, its excess
    over the ceiling printed and asserted below 0.2 dB, the tolerance tests/test_truepeak_emu.py grants the meter itself"""
    assert len(randoms) == 300
    worst = (0.0, 0, None)
    for kind, x, ceiling, S in randoms:
        cfgs, p = _mono(x)
        o, e = LM.Oracle(cfgs, ceiling, steps=[S]), LM.LimiterEmu(cfgs, ceiling, steps=[S])
        want = o.limit(p)
        _check(e.limit(p), want, (kind, ceiling, S))
        y = want[0]
        assert (32768 * np.abs(y[:, 0, 0].astype(np.int64)) <= ceiling).all(), (kind, ceiling, S)
        tp = TP.Oracle(cfgs, ceiling).truepeak(y)
        peak = int(tp["peak_max"][0, 0])
        excess = TP.dbtp(peak) - TP.dbtp(ceiling) if peak > ceiling else 0.0
        if excess > worst[0]:
            worst = (excess, peak - ceiling, (kind, ceiling, S))
        assert excess < 0.2, (kind, ceiling, S, excess)
    print("worst true-peak excess over the ceiling: %.5f dB, %d units of 2^-30, %s" % worst)


def test_a_signal_at_or_below_the_ceiling_comes_out_as_itself(randoms):
    """the ceiling set to the signal's own maximum P: nothing is over, the output is the input 63 samples late; one unit lower, it is not"""
    for kind, x, _, S in randoms[:10]:
        cfgs, p = _mono(x)
        P = int(TP.Oracle(cfgs).truepeak(p)["peak_max"][0, 0])
        if not (1 << 20) <= P <= (1 << 30):
            continue
        want = LM.Oracle(cfgs, P, steps=[S]).limit(p)
        _check(LM.LimiterEmu(cfgs, P, steps=[S]).limit(p), want, kind)
        assert np.array_equal(want[0][:, 0, 0].reshape(-1)[63:], x[:-63]) and not want[1]["limited"][0] and want[1]["peak_in_max"][0] == P
        if P > (1 << 20):
            lower = LM.Oracle(cfgs, P - 1, steps=[S]).limit(p)
            _check(LM.LimiterEmu(cfgs, P - 1, steps=[S]).limit(p), lower, kind)
            assert lower[1]["limited"][0]


@pytest.mark.parametrize("ceiling", [0, 1 << 29], ids=["-1 dBTP", "-6 dBTP"])
def test_structured_signals_leave_at_or_below_the_ceiling_in_true_peak(ceiling):
    """EBU Tech 3341's fs/4 sine at 45 degrees, the 1 kHz burst, a 100 Hz sine, a period-14 square, a sweep, gated sines and Nyquist
    squares, all at full scale: the output's true peak, by the meter's oracle at the same ceiling, has no over"""
    for name, x in LM.structured():
        cfgs, p = _mono(x)
        want = LM.Oracle(cfgs, ceiling).limit(p)
        _check(LM.LimiterEmu(cfgs, ceiling).limit(p), want, name)
        assert want[1]["limited"][0], name
        tp = TP.Oracle(cfgs, ceiling).truepeak(want[0])
        assert tp["overs"][0] == 0, (name, int(tp["peak_max"][0, 0]), ceiling)


def test_sanitized_program():
    """tests/emu/limiter_sanitize_main.cpp: the emulation over 37 streams and over one, both paths, the slots flush against the end of their
    allocations, under AddressSanitizer + UBSan, built and run as a program of its own"""
    exe = LM.build_sanitized()
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
