"""The true-peak meter on the GPU (csrc/toolame_truepeak.hip, tlb_truepeak_* / tlb_tick_*truepeak* / tlb_node_*truepeak*): the device against
the emulation of tests/truepeaklib.py byte for byte on the 37-stream, 45-frame case with the constructed cases appended as extra streams, in
the three cuts; the life-cycle calls and the argument checks; a tick object with the meter against one without (byte-identical output) and
against the emulation after every wait, in both loops with 1 and 3 groups, once with the loudness meter on as well; resets in mid-run;
the node level with a restarted shard."""
import numpy as np
import pytest

import truepeaklib as TP

pytestmark = pytest.mark.gpu
N = TP.N


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def case(M):
    """(S, PCM): the 37 streams and, behind them, the constructed cases (their signals in the first frames, silence after)"""
    cc, cx, _ = TP.constructed(TP.NFRAMES)
    return TP.STREAMS + cc, np.concatenate([TP.pcm_of(TP.STREAMS), cx], axis=1)


@pytest.fixture(scope="module")
def emu(case):
    """the emulation's records after every frame (run frame by frame: the CPU tests show that the cut does not matter)"""
    S, PCM = case
    e = TP.TruePeakEmu(S)
    return [e.truepeak(PCM[f:f + 1]) for f in range(TP.NFRAMES)]


def _same(got, want):
    """a binding record array against a truepeaklib one: same layout, same bytes"""
    assert got.dtype.itemsize == want.dtype.itemsize and got.dtype.names == want.dtype.names
    return got.tobytes() == want.tobytes()


def _diff(got, want):
    return [s for s in range(len(got)) if got[s].tobytes() != want[s].tobytes()][:6]


@pytest.mark.parametrize("cuts", TP.CUTS, ids=["one", "frames", "7+38"])
def test_device_equals_emulation(M, case, emu, cuts):
    S, PCM = case
    b = M.Batch(TP.stream_configs(S))
    b.enable_truepeak()
    b.enable_truepeak(12345)                                         # a second call answers OK and leaves the ceiling
    f0 = 0
    for n in cuts:
        got = b.truepeak(PCM[f0:f0 + n])
        f0 += n
        assert _same(got, emu[f0 - 1]), (cuts, f0, _diff(got, emu[f0 - 1]))
    assert M.TRUEPEAK_DTYPE.itemsize == 32
    assert got["overs"].any() and not got["overs"].all() and (got["peak_max"][:, 0] >= 32768 * got["sample_max"][:, 0]).all()
    b.close()


def test_a_peak_at_the_ceiling_is_not_an_over_and_one_above_it_is(M, case, emu):
    """the ceiling at enable time: stream 0's maximum peak P itself (no over), P - 1 (the frames that reach P are)"""
    S, PCM = case
    P = int(emu[5]["peak_max"][0].max())
    for ceiling in (P, P - 1):
        b, e = M.Batch(TP.stream_configs(S[:3])), TP.TruePeakEmu(S[:3], ceiling)
        b.enable_truepeak(ceiling)
        got, want = b.truepeak(PCM[:6, :3]), e.truepeak(PCM[:6, :3])
        assert _same(got, want) and (got["overs"][0] > 0) == (ceiling < P), (ceiling, got["overs"])
        b.close()


def test_life_cycle(M, case):
    """truepeak_reset of one stream and of all, tlb_stream_reset, tlb_stream_reconfigure to another rate and channel count; tlb_stream_finish
    leaves the meter alone"""
    S, PCM = case
    new = dict(samplerate=16000, mode="m")
    b, e = M.Batch(TP.stream_configs(S)), TP.TruePeakEmu(S)
    b.enable_truepeak()
    assert _same(b.truepeak(PCM[:12]), e.truepeak(PCM[:12]))
    b.truepeak_reset(3); e.reset(3)
    b.stream_reset(5); e.reset(5)
    b.stream_reconfigure(8, TP.stream_configs([new])[0]); e.reconfigure(8, new)
    b.stream_finish(9)
    got, want = b.truepeak(PCM[12:20]), e.truepeak(PCM[12:20])
    assert _same(got, want), _diff(got, want)
    assert [int(got["frames"][s]) for s in (3, 5, 8, 9, 10)] == [8, 8, 8, 20, 20]
    assert not got["peak_max"][8, 1] and got["peak_max"][8, 0]
    b.truepeak_reset(); e.reset(-1)
    assert _same(b.truepeak(PCM[20:21]), e.truepeak(PCM[20:21]))
    b.close()


def test_argument_checks_and_opt_in(M, case):
    """a batch that never enabled the meter refuses the calls (TLB_ERR_ARG) and its life-cycle calls do what they did; bad arguments change
    nothing"""
    S, PCM = case
    b = M.Batch(TP.stream_configs(S[:3]))
    for call in (lambda: b.truepeak(PCM[:1, :3]), b.truepeak_reset):
        with pytest.raises(M.ToolameError) as err:
            call()
        assert err.value.code == 18
    b.stream_reset(0); b.stream_finish(1)
    b.enable_truepeak()
    L = b.L
    rec = np.zeros(3, dtype=M.TRUEPEAK_DTYPE)
    assert L.tlb_truepeak_host(b.h, None, 1, rec.ctypes.data) == 18 and L.tlb_truepeak_host(b.h, PCM.ctypes.data, 0, rec.ctypes.data) == 18
    assert L.tlb_truepeak_device(b.h, 16 + 2, 1, None, None) == 18                      # a misaligned device pointer is refused before it is used
    assert L.tlb_truepeak_device(b.h, None, 1, None, None) == 18 and L.tlb_truepeak_device(b.h, 4096, 0, None, None) == 18
    assert L.tlb_truepeak_reset(b.h, 3) == 18 and L.tlb_truepeak_reset(b.h, -2) == 18
    e = TP.TruePeakEmu(S[:3])
    assert _same(b.truepeak(PCM[:2, :3]), e.truepeak(PCM[:2, :3]))
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
TS = TP.STREAMS[:13]                                                 # the tick and node cases: every rate twice, one and two channels
T = 9


@pytest.fixture(scope="module")
def tick_in(M):
    """what the caller hands in, int16 [T][ns][2304] interleaved (a one-channel stream is its first 1152 values), and the planar PCM the
    ingest makes of it, which is what the meter is defined on"""
    planar = TP.pcm_of(TS, T)
    inter = np.zeros((T, len(TS), 2 * N), dtype=np.int16)
    for s, c in enumerate(TS):
        if TP.nch_of(c) == 2:
            inter[:, s] = planar[:, s].transpose(0, 2, 1).reshape(T, -1)
        else:
            inter[:, s, :N] = planar[:, s, 0]
            inter[:, s, N:] = 0x1234
    b = M.Batch(TP.stream_configs(TS))
    got, _ = b.ingest(inter)
    b.close()
    for s, c in enumerate(TS):
        assert np.array_equal(got[:, s, :TP.nch_of(c)], planar[:, s, :TP.nch_of(c)]), s
    return inter, got


def _loop(t, inter, pipelined, after, before=None):
    """the ticks of `inter` in either loop -- run(), or submit, submit, wait ... -- then finish; after(i) follows every wait, after(T) the finish"""
    n, done = inter.shape[0], 0
    for f in range(n):
        if before:
            before(f)
        t.pcm[:] = inter[f]
        if not pipelined:
            t.run()
            after(done); done += 1
        else:
            t.submit()
            if f >= 1:
                t.wait()
                after(done); done += 1
    if pipelined:
        t.wait()
        after(done); done += 1
    assert done == n
    t.finish()
    after(n)


def _snap(t, ns):
    return [(t.frame(s), tuple(int(x) for x in t.peaks[s]), int(t.silence_ms[s])) for s in range(ns)]


@pytest.mark.parametrize("ngroups,pipelined,loud", [(1, False, False), (3, True, False), (3, False, True), (1, True, False)])
def test_tick_with_truepeak_against_one_without_and_against_the_emulation(M, tick_in, ngroups, pipelined, loud):
    """packets, peaks and silence counters byte for byte; after EVERY wait Tick.truepeak equals the emulation run over the PCM handed in so
    far; the finish adds nothing.  loud: the loudness meter is on as well, and its records are those of a tick object without true peak"""
    import loudnesslib as LL
    inter, planar = tick_in
    cfgs, ns = TP.stream_configs(TS), len(TS)
    snaps, louds = [], []
    for on in (False, True):
        t = M.Tick(cfgs, egress="frames", ngroups=ngroups)
        e = TP.TruePeakEmu(TS)
        got, want, lrec = [], [], []
        if loud:
            t.enable_loudness()
        if on:
            t.enable_truepeak()
            t.enable_truepeak()
            assert not t.truepeak.view(np.uint8).any()

        def after(i):
            got.append(_snap(t, ns))
            if loud:
                lrec.append(t.loudness.tobytes())
            if not on:
                assert t.truepeak is None
                return
            if i < T:
                want.append(e.truepeak(planar[i:i + 1]))
            assert _same(t.truepeak, want[-1]), (i, _diff(t.truepeak, want[-1]))

        _loop(t, inter, pipelined, after)
        if on:
            assert list(t.truepeak["frames"]) == [T] * ns and t.truepeak["peak_max"].any()
        if loud:
            le = LL.LoudnessEmu(TS)
            assert t.loudness.tobytes() == le.loudness(planar).tobytes()
        t.close()
        snaps.append(got); louds.append(lrec)
    assert len(snaps[0]) == T + 1 and all(len(x[0]) > 0 for x in snaps[0][1])
    assert snaps[1] == snaps[0] and louds[1] == louds[0]


def test_tick_stream_reset_and_truepeak_reset_in_mid_run(M, tick_in):
    """tlb_tick_stream_reset of stream 4 before tick 3 and tlb_tick_truepeak_reset of stream 11 before tick 5 (another group): each starts
    over there, every other stream's records are those of the emulation undisturbed; the calls are refused with a tick in flight"""
    inter, planar = tick_in
    t, e = M.Tick(TP.stream_configs(TS), egress="frames", ngroups=3), TP.TruePeakEmu(TS)
    t.enable_truepeak()

    def before(f):
        if f == 3:
            t.stream_reset(4); e.reset(4)
        if f == 5:
            t.truepeak_reset(11); e.reset(11)

    def after(i):
        if i < T:
            want = e.truepeak(planar[i:i + 1])
            assert _same(t.truepeak, want), i

    _loop(t, inter, False, after, before)
    assert [int(t.truepeak["frames"][s]) for s in (3, 4, 11)] == [T, T - 3, T - 5]
    t.close()
    t = M.Tick(TP.stream_configs(TS[:4]), egress="frames")
    t.enable_truepeak(1 << 26)
    t.pcm[:] = inter[0, :4]
    t.submit()
    assert t.L.tlb_tick_truepeak_reset(t.h, 0) == 18                 # a tick is in flight
    t.wait()
    e = TP.TruePeakEmu(TS[:4], 1 << 26)
    assert _same(t.truepeak, e.truepeak(planar[:1, :4]))             # the ceiling given at enable time is the one in force: -24 dBTP, which the
    assert list(t.truepeak["overs"]) == [1, 1, 1, 0]                 # noise at -20 dBFS passes and the default's -1 dBTP would not count
    assert t.L.tlb_tick_enable_truepeak(t.h, 0) == 18                # the opt-in calls are for before the first submit, even when already on
    assert t.L.tlb_tick_truepeak_reset(t.h, 4) == 18 and t.L.tlb_tick_truepeak_reset(t.h, -2) == 18
    t.truepeak_reset()
    t.close()
    u = M.Tick(TP.stream_configs(TS[:4]), egress="frames")           # never enabled: NULL, refused, and enabling after the first submit refused
    u.pcm[:] = inter[0, :4]
    u.run()
    assert u.truepeak is None and u.L.tlb_tick_enable_truepeak(u.h, 0) == 18 and u.L.tlb_tick_truepeak_reset(u.h, -1) == 18
    u.close()


def test_node_truepeak(M, tick_in):
    """two shards on the one GPU: records by node-wide index equal the emulation's; with the fault-injection build present, a broken
    shard's streams answer NULL while the others carry on, and a restarted shard measures again from zero with the same ceiling; a BATCH
    node refuses"""
    inter, planar = tick_in
    ns = len(TS)
    ceiling = 1 << 26                                                # -24 dBTP: stream 8's noise at -20 dBFS is over this and under the default, so a restarted
                                                                     # shard that came back with the default would differ from the emulation
    fi = M.load_fault_library() if M.FAULT_LIB_PATH.exists() else None
    nd = M.Node(TP.stream_configs(TS), devices=(0, 0), plane="tick", egress="frames", ngroups=2, lib=fi)
    e = TP.TruePeakEmu(TS, ceiling)
    assert nd.truepeak(0) is None
    nd.enable_truepeak(ceiling)
    nd.enable_truepeak()
    (f1, n1) = nd.blocks[1]
    mine = [s for s in range(ns) if f1 <= s < f1 + n1]
    others = [s for s in range(ns) if s not in mine]
    assert mine and others

    def step(f, check):
        nd.set_pcm(inter[f])
        nd.run()
        want = e.truepeak(planar[f:f + 1])
        for s in check:
            assert nd.truepeak(s).tobytes() == want[s].tobytes(), (f, s)

    for f in range(4):
        step(f, range(ns))
    nd.truepeak_reset(2); e.reset(2)
    if fi is not None:
        nd.fail_next(1, 1)
        nd.set_pcm(inter[4])
        with pytest.raises(M.ToolameError) as err:
            nd.run()
        assert err.value.code == 17 and not nd.shard_ok(1)
        want = e.truepeak(planar[4:5])
        for s in range(ns):
            assert (nd.truepeak(s) is None) if s in mine else (nd.truepeak(s).tobytes() == want[s].tobytes()), s
        with pytest.raises(M.ToolameError) as err:
            nd.truepeak_reset(f1)
        assert err.value.code == 17
        step(5, others)
        assert all(nd.truepeak(s) is None for s in mine)
        nd.shard_restart(1)
        for s in mine:
            assert nd.truepeak(s).tobytes() == bytes(32)             # from zero: its streams are fresh
            e.reset(s)
        for f in (6, 7, 8):
            step(f, range(ns))
        assert [int(nd.truepeak(s)["frames"]) for s in (others[0], mine[0])] == [T if others[0] != 2 else T - 4, 3]
        assert 8 in mine and int(nd.truepeak(8)["overs"]) == 3
    else:
        for f in range(4, T):
            step(f, range(ns))
    nd.close()
    b = M.Node(TP.stream_configs(TS), devices=(0, 0), plane="batch")
    assert b.L.tlb_node_enable_truepeak(b.h, 0) == 18 and b.truepeak(0) is None and b.L.tlb_node_truepeak_reset(b.h, 0) == 18
    b.close()
