"""The loudness meter on the GPU (csrc/toolame_loudness.hip, tlb_loudness_* / tlb_tick_*loudness* / tlb_node_*loudness*): the device against
the emulation of tests/loudnesslib.py bit for bit on the 37-stream, 45-frame case in the three cuts, the life-cycle calls and the argument
checks; a tick object with loudness against one without (byte-identical output) and against the emulation after every wait, in both loops
with 1 and 3 groups; a stream reset in mid-run; the node level with a restarted shard."""
import numpy as np
import pytest

import loudnesslib as LL

pytestmark = pytest.mark.gpu
S = LL.STREAMS
NS = len(S)


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def pcm():
    return LL.pcm_of(S)


@pytest.fixture(scope="module")
def emu(pcm):
    """the emulation's records after every frame (run frame by frame: the CPU tests show that the cut does not matter) and its programme"""
    e = LL.LoudnessEmu(S)
    recs = [e.loudness(pcm[f:f + 1]) for f in range(LL.NFRAMES)]
    return recs, e.programme()


def _same(M, got, want):
    """a binding record array against a loudnesslib one: same layout, same bytes"""
    assert got.dtype.itemsize == want.dtype.itemsize and got.dtype.names == want.dtype.names
    return got.tobytes() == want.tobytes()


@pytest.mark.parametrize("cuts", LL.CUTS, ids=["one", "frames", "7+38"])
def test_device_equals_emulation(M, pcm, emu, cuts):
    recs, prog = emu
    b = M.Batch(LL.stream_configs(S))
    b.enable_loudness()
    b.enable_loudness()                                              # a second call answers OK
    f0 = 0
    for n in cuts:
        got = b.loudness(pcm[f0:f0 + n])
        f0 += n
        assert _same(M, got, recs[f0 - 1]), (cuts, f0, [s for s in range(NS) if got[s].tobytes() != recs[f0 - 1][s].tobytes()][:6])
    assert _same(M, b.loudness_programme(), prog)
    assert M.LOUDNESS_DTYPE.itemsize == 48 and M.LOUDNESS_PROGRAMME_DTYPE.itemsize == 24
    b.close()


def test_life_cycle(M, pcm):
    """loudness_reset of one stream and of all, tlb_stream_reset, tlb_stream_reconfigure to another rate and channel count; tlb_stream_finish
    leaves the meter alone"""
    new = dict(samplerate=16000, mode="m")
    b, e = M.Batch(LL.stream_configs(S)), LL.LoudnessEmu(S)
    b.enable_loudness()
    assert _same(M, b.loudness(pcm[:12]), e.loudness(pcm[:12]))
    b.loudness_reset(3); e.reset(3)
    b.stream_reset(5); e.reset(5)
    b.stream_reconfigure(8, LL.stream_configs([new])[0]); e.reconfigure(8, new)
    b.stream_finish(9)
    got, want = b.loudness(pcm[12:20]), e.loudness(pcm[12:20])
    assert _same(M, got, want)
    assert [int(got["frames"][s]) for s in (3, 5, 8, 9, 10)] == [8, 8, 8, 20, 20]
    assert _same(M, b.loudness_programme(), e.programme())
    b.loudness_reset(); e.reset(-1)
    assert _same(M, b.loudness(pcm[20:21]), e.loudness(pcm[20:21]))
    assert _same(M, b.loudness_programme(), e.programme())
    b.close()


def test_argument_checks_and_opt_in(M, pcm):
    """a batch that never enabled loudness refuses the calls (TLB_ERR_ARG) and its life-cycle calls do what they did; bad arguments change
    nothing"""
    b = M.Batch(LL.stream_configs(S[:3]))
    for call in (lambda: b.loudness(pcm[:1, :3]), b.loudness_programme, b.loudness_reset):
        with pytest.raises(M.ToolameError) as err:
            call()
        assert err.value.code == 18
    b.stream_reset(0); b.stream_finish(1)
    b.enable_loudness()
    L = b.L
    rec = np.zeros(3, dtype=M.LOUDNESS_DTYPE)
    assert L.tlb_loudness_host(b.h, None, 1, rec.ctypes.data) == 18 and L.tlb_loudness_host(b.h, pcm.ctypes.data, 0, rec.ctypes.data) == 18
    assert L.tlb_loudness_device(b.h, 16 + 2, 1, None, None) == 18                      # a misaligned device pointer is refused before it is used
    assert L.tlb_loudness_reset(b.h, 3) == 18 and L.tlb_loudness_reset(b.h, -2) == 18
    e = LL.LoudnessEmu(S[:3])
    assert _same(M, b.loudness(pcm[:2, :3]), e.loudness(pcm[:2, :3]))
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
TS = S[:13]                                                          # the tick and node cases: every rate twice, one and two channels
T = 9                                                                # 10 368 samples: 6 bins at 16 kHz (momentary exists from 24 kHz down), 2 at 48 kHz


@pytest.fixture(scope="module")
def tick_in(M):
    """what the caller hands in, int16 [T][ns][2304] interleaved (a one-channel stream is its first 1152 values), and the planar PCM the
    ingest makes of it, which is what the meter is defined on"""
    planar = LL.pcm_of(TS, T)
    inter = np.zeros((T, len(TS), 2 * LL.N), dtype=np.int16)
    for s, c in enumerate(TS):
        if LL.nch_of(c) == 2:
            inter[:, s] = planar[:, s].transpose(0, 2, 1).reshape(T, -1)
        else:
            inter[:, s, :LL.N] = planar[:, s, 0]
            inter[:, s, LL.N:] = 0x1234
    b = M.Batch(LL.stream_configs(TS))
    got, _ = b.ingest(inter)
    b.close()
    for s, c in enumerate(TS):
        assert np.array_equal(got[:, s, :LL.nch_of(c)], planar[:, s, :LL.nch_of(c)]), s
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


@pytest.mark.parametrize("ngroups,pipelined", [(1, False), (3, True), (3, False), (1, True)])
def test_tick_with_loudness_against_one_without_and_against_the_emulation(M, tick_in, ngroups, pipelined):
    """packets byte for byte; after EVERY wait Tick.loudness equals the emulation run over the PCM handed in so far; the finish adds nothing"""
    inter, planar = tick_in
    cfgs, ns = LL.stream_configs(TS), len(TS)
    snaps = []
    for on in (False, True):
        t = M.Tick(cfgs, egress="frames", ngroups=ngroups)
        e = LL.LoudnessEmu(TS)
        got, want = [], []
        if on:
            t.enable_loudness()
            t.enable_loudness()
            assert not t.loudness.view(np.uint8).any()

        def after(i):
            got.append(_snap(t, ns))
            if not on:
                assert t.loudness is None
                return
            if i < T:
                want.append(e.loudness(planar[i:i + 1]))
            assert _same(M, t.loudness, want[-1]), (i, [s for s in range(ns) if t.loudness[s].tobytes() != want[-1][s].tobytes()])

        _loop(t, inter, pipelined, after)
        if on:
            assert list(t.loudness["frames"]) == [T] * ns and (t.loudness["momentary"] > 0).any()
            assert _same(M, t.loudness_programme(), e.programme())
        t.close()
        snaps.append(got)
    assert len(snaps[0]) == T + 1 and all(len(x[0]) > 0 for x in snaps[0][1])
    assert snaps[1] == snaps[0]


def test_tick_stream_reset_and_loudness_reset_in_mid_run(M, tick_in):
    """tlb_tick_stream_reset of stream 4 before tick 3 and tlb_tick_loudness_reset of stream 11 before tick 5 (another group): each starts
    over there, every other stream's records are those of the emulation undisturbed; the calls are refused with a tick in flight"""
    inter, planar = tick_in
    ns = len(TS)
    t, e = M.Tick(LL.stream_configs(TS), egress="frames", ngroups=3), LL.LoudnessEmu(TS)
    t.enable_loudness()

    def before(f):
        if f == 3:
            t.stream_reset(4); e.reset(4)
        if f == 5:
            t.loudness_reset(11); e.reset(11)

    def after(i):
        if i < T:
            want = e.loudness(planar[i:i + 1])
            assert _same(M, t.loudness, want), i

    _loop(t, inter, False, after, before)
    assert [int(t.loudness["frames"][s]) for s in (3, 4, 11)] == [T, T - 3, T - 5]
    t.close()
    t = M.Tick(LL.stream_configs(TS[:4]), egress="frames")
    t.enable_loudness()
    t.pcm[:] = inter[0, :4]
    t.submit()
    prog = np.zeros(4, dtype=M.LOUDNESS_PROGRAMME_DTYPE)
    assert t.L.tlb_tick_loudness_reset(t.h, 0) == 18 and t.L.tlb_tick_loudness_programme(t.h, prog.ctypes.data) == 18      # a tick is in flight
    t.wait()
    assert t.L.tlb_tick_enable_loudness(t.h) == 18                   # the opt-in calls are for before the first submit, even when already on
    assert t.L.tlb_tick_loudness_reset(t.h, 4) == 18 and t.L.tlb_tick_loudness_reset(t.h, -2) == 18
    t.loudness_reset(); t.loudness_programme()
    t.close()
    u = M.Tick(LL.stream_configs(TS[:4]), egress="frames")           # never enabled: NULL, refused, and enabling after the first submit refused
    u.pcm[:] = inter[0, :4]
    u.run()
    assert u.loudness is None and u.L.tlb_tick_enable_loudness(u.h) == 18 and u.L.tlb_tick_loudness_reset(u.h, -1) == 18
    assert u.L.tlb_tick_loudness_programme(u.h, prog.ctypes.data) == 18
    u.close()


def test_node_loudness(M, tick_in):
    """two shards on the one GPU: records by node-wide index equal the emulation's; with the fault-injection build present, a broken
    shard's streams answer NULL while the others carry on, and a restarted shard measures again from zero; a BATCH node refuses"""
    inter, planar = tick_in
    ns = len(TS)
    fi = M.load_fault_library() if M.FAULT_LIB_PATH.exists() else None
    nd = M.Node(LL.stream_configs(TS), devices=(0, 0), plane="tick", egress="frames", ngroups=2, lib=fi)
    e = LL.LoudnessEmu(TS)
    assert nd.loudness(0) is None
    nd.enable_loudness()
    nd.enable_loudness()
    (f1, n1) = nd.blocks[1]
    mine = [s for s in range(ns) if f1 <= s < f1 + n1]
    others = [s for s in range(ns) if s not in mine]
    assert mine and others

    def step(f, check):
        nd.set_pcm(inter[f])
        nd.run()
        want = e.loudness(planar[f:f + 1])
        for s in check:
            assert nd.loudness(s).tobytes() == want[s].tobytes(), (f, s)

    for f in range(4):
        step(f, range(ns))
    assert _same(M, nd.loudness_programme(), e.programme())
    nd.loudness_reset(2); e.reset(2)
    if fi is not None:
        nd.fail_next(1, 1)
        nd.set_pcm(inter[4])
        with pytest.raises(M.ToolameError) as err:
            nd.run()
        assert err.value.code == 17 and not nd.shard_ok(1)
        want = e.loudness(planar[4:5])
        for s in range(ns):
            assert (nd.loudness(s) is None) if s in mine else (nd.loudness(s).tobytes() == want[s].tobytes()), s
        with pytest.raises(M.ToolameError) as err:
            nd.loudness_reset(f1)
        assert err.value.code == 17
        step(5, others)
        assert all(nd.loudness(s) is None for s in mine)
        nd.shard_restart(1)
        for s in mine:
            assert nd.loudness(s).tobytes() == bytes(48)             # from zero: its streams are fresh
            e.reset(s)
        for f in (6, 7, 8):
            step(f, range(ns))
        assert [int(nd.loudness(s)["frames"]) for s in (others[0], mine[0])] == [T if others[0] != 2 else T - 4, 3]
    else:
        for f in range(4, T):
            step(f, range(ns))
    assert _same(M, nd.loudness_programme(), e.programme())
    nd.close()
    b = M.Node(LL.stream_configs(TS), devices=(0, 0), plane="batch")
    assert b.L.tlb_node_enable_loudness(b.h) == 18 and b.loudness(0) is None and b.L.tlb_node_loudness_reset(b.h, 0) == 18
    b.close()
