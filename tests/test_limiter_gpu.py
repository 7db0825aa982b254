"""The true-peak limiter on the GPU (csrc/toolame_limiter.hip, tlb_limiter_* / tlb_tick_*limiter* / tlb_node_*limiter*): six streams by
four frames carrying the constructed cases of tests/limiterlib.py, the device against the emulation against the definition, byte for byte
on the PCM and on the records, in one call and frame by frame; the life-cycle calls and the argument checks; a tick object with the
limiter against the batch-plane chain ingest, limit, encode, and one without it against the chain without it; the node level with records
routed per stream and a restarted shard; and the true-peak meter beside the limiter at the same ceiling on the structured burst."""
import numpy as np
import pytest

import limiterlib as LM
import truepeaklib as TP

pytestmark = pytest.mark.gpu
N = LM.N
T = 6


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def case():
    cfgs, x, names = LM.constructed(4)
    return cfgs, x


@pytest.fixture(scope="module")
def ref(case):
    """per (ceiling, release): the oracle's PCM and its records after every frame, and the emulation's, which must be the same"""
    cfgs, x = case
    out = {}
    for key in ((0, 0), (300000000, 1), (1 << 20, 5)):
        o, e = LM.Oracle(cfgs, *key), LM.LimiterEmu(cfgs, *key)
        pcm, recs = [], []
        for f in range(x.shape[0]):
            wp, wr = o.limit(x[f:f + 1])
            gp, gr = e.limit(x[f:f + 1])
            assert np.array_equal(gp, wp) and LM.same(gr, wr)
            pcm.append(wp); recs.append(wr)
        out[key] = (np.concatenate(pcm), recs)
    return out


def _same(got, want):
    """a binding record array against a limiterlib one: same layout, same bytes"""
    assert got.dtype.itemsize == want.dtype.itemsize and got.dtype.names == want.dtype.names
    return got.tobytes() == want.tobytes()


def _diff(got, want):
    return [(s, got[s], want[s]) for s in range(len(got)) if got[s].tobytes() != want[s].tobytes()][:3]


@pytest.mark.parametrize("cuts", [(4,), (1, 1, 1, 1), (3, 1)], ids=["one", "frames", "3+1"])
@pytest.mark.parametrize("key", [(0, 0), (300000000, 1), (1 << 20, 5)], ids=["default", "300M 1ms", "2^20 5ms"])
def test_device_equals_emulation_equals_definition(M, case, ref, key, cuts):
    cfgs, x = case
    want_pcm, want_rec = ref[key]
    b = M.Batch(LM.LL.stream_configs(cfgs))
    b.enable_limiter(*key)
    b.enable_limiter(*key)                                           # equal parameters: OK
    with pytest.raises(M.ToolameError) as err:
        b.enable_limiter(1 << 25, 7)
    assert err.value.code == 18
    f0 = 0
    for n in cuts:
        got, rec = b.limit(x[f0:f0 + n])
        bad = [s for s in range(len(cfgs)) if not np.array_equal(got[:, s], want_pcm[f0:f0 + n, s])]
        assert not bad, (key, cuts, f0, bad)
        f0 += n
        assert _same(rec, want_rec[f0 - 1]), (key, cuts, f0, _diff(rec, want_rec[f0 - 1]))
    assert M.LIMITER_DTYPE.itemsize == 32 and rec["limited"].any() and (rec["frames"] == 4).all()
    assert (got[:, 0, 1] == 0x5a5a).all()                            # a one-channel stream's second row is neither read nor written
    b.close()


def test_life_cycle_and_argument_checks(M, case, ref):
    """a batch that never enabled the limiter refuses the calls; limiter_reset, tlb_stream_reset and tlb_stream_reconfigure (another rate:
    another S, and one channel) start the stream over, tlb_stream_finish leaves it; bad arguments change nothing"""
    cfgs, x = case
    b = M.Batch(LM.LL.stream_configs(cfgs))
    for call in (lambda: b.limit(x[:1]), b.limiter_reset):
        with pytest.raises(M.ToolameError) as err:
            call()
        assert err.value.code == 18
    L = b.L
    bad = np.array([1 << 19, 0], dtype=np.uint32)
    assert L.tlb_limiter_enable(b.h, bad.ctypes.data) == 18
    bad[:] = (0, 10001)
    assert L.tlb_limiter_enable(b.h, bad.ctypes.data) == 18
    assert L.tlb_limiter_enable(b.h, None) == 0                      # NULL: both defaults
    b.enable_limiter(M.TRUEPEAK_CEILING_DEFAULT, 100)                # ... which is what these name
    rec = np.zeros(len(cfgs), dtype=M.LIMITER_DTYPE)
    assert L.tlb_limiter_host(b.h, None, 1, rec.ctypes.data) == 18 and L.tlb_limiter_host(b.h, x.ctypes.data, 0, rec.ctypes.data) == 18
    assert L.tlb_limiter_device(b.h, 16 + 2, 1, None, None) == 18    # a misaligned device pointer is refused before it is used
    assert L.tlb_limiter_device(b.h, None, 1, None, None) == 18 and L.tlb_limiter_device(b.h, 4096, 0, None, None) == 18
    assert L.tlb_limiter_reset(b.h, len(cfgs)) == 18 and L.tlb_limiter_reset(b.h, -2) == 18
    o, e = LM.Oracle(cfgs), LM.LimiterEmu(cfgs)
    got, want = b.limit(x[:2]), o.limit(x[:2])
    assert np.array_equal(got[0], want[0]) and _same(got[1], want[1])
    new = dict(samplerate=16000, mode="m")
    b.limiter_reset(0); o.reset(0)
    b.stream_reset(2); o.reset(2)
    b.stream_reconfigure(3, LM.LL.stream_configs([new])[0]); o.reconfigure(3, new)
    b.stream_finish(4)
    got, want = b.limit(x[2:]), o.limit(x[2:])
    assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]), _diff(got[1], want[1])
    assert [int(got[1]["frames"][s]) for s in (0, 2, 3, 4, 5)] == [2, 2, 2, 4, 4]
    assert np.array_equal(got[0][:, 3, 1], x[2:, 3, 1])              # stream 3 has one channel now
    b.limiter_reset(); o.reset(-1)
    got, want = b.limit(x[:1]), o.limit(x[:1])
    assert np.array_equal(got[0], want[0]) and _same(got[1], want[1])
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tick_in(M):
    """what the caller hands in, int16 [T][6][2304] interleaved (a one-channel stream is its first 1152 values), and the planar PCM the
    ingest makes of it, which is what the limiter is defined on"""
    cfgs, planar, _ = LM.constructed(T)
    inter = np.zeros((T, len(cfgs), 2 * N), dtype=np.int16)
    for s, c in enumerate(cfgs):
        if LM.nch_of(c) == 2:
            inter[:, s] = planar[:, s].transpose(0, 2, 1).reshape(T, -1)
        else:
            inter[:, s, :N] = planar[:, s, 0]
    return cfgs, inter


@pytest.fixture(scope="module")
def chains(M, tick_in):
    """the batch-plane chains, once: ingest then encode, and ingest, limit, encode -> per chain (frames per stream and tick with the
    flushed frame last, the ingest's peaks, the limiter's records after every tick)"""
    cfgs, inter = tick_in
    out = {}
    for on in (False, True):
        b = M.Batch(LM.LL.stream_configs(cfgs))
        if on:
            b.enable_limiter(0, 20)
        frames, recs, peaks = [[] for _ in cfgs], [], []
        for f in range(T):
            planar, pk = b.ingest(inter[f:f + 1])
            if on:
                planar, rec = b.limit(planar)
                recs.append(rec)
            got, _ = b.encode(planar)
            for s in range(len(cfgs)):
                if got[s]:
                    frames[s].append(bytes(got[s]))
            peaks.append(np.array(pk[0]))
        tail = b.flush()
        for s in range(len(cfgs)):
            frames[s].append(bytes(tail[s]))
        b.close()
        out[on] = (frames, peaks, recs)
    assert out[True][0] != out[False][0]                             # the limiter changes what is encoded
    return out


def _loop(t, inter, pipelined, after):
    """the ticks of `inter` in either loop -- run(), or submit, submit, wait ... -- then finish; after(i) follows every wait, after(n) the finish"""
    n, done = inter.shape[0], 0
    for f in range(n):
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


@pytest.mark.parametrize("on,ngroups,pipelined", [(True, 1, False), (True, 3, True), (False, 2, False)], ids=["on 1 group", "on 3 groups pipelined", "off"])
def test_tick_against_the_batch_plane_chain(M, tick_in, chains, on, ngroups, pipelined):
    """frames, peaks and records of every tick byte for byte: with the limiter, those of ingest, limit, encode; without it, those of ingest,
    encode (what the object gave before) and no records.  The ingest's peaks are the INPUT's either way; the finish adds no record"""
    cfgs, inter = tick_in
    frames, peaks, recs = chains[on]
    ns = len(cfgs)
    t = M.Tick(LM.LL.stream_configs(cfgs), egress="frames", ngroups=ngroups)
    if on:
        t.enable_limiter(0, 20)
        t.enable_limiter(0, 20)
        assert t.L.tlb_tick_enable_limiter(t.h, np.array([0, 21], dtype=np.uint32).ctypes.data) == 18
        assert not t.limiter.view(np.uint8).any()
    got = [[] for _ in range(ns)]

    def after(i):
        for s in range(ns):
            fr = t.frame(s)
            if fr:
                got[s].append(fr)
        if i < T:
            assert np.array_equal(np.array(t.peaks).reshape(ns, 2), peaks[i].reshape(ns, 2)), i
        if not on:
            assert t.limiter is None
        else:
            want = recs[min(i, T - 1)]
            assert _same(t.limiter, want), (i, _diff(t.limiter, want))

    _loop(t, inter, pipelined, after)
    assert got == frames
    if on:
        assert list(t.limiter["frames"]) == [T] * ns and t.limiter["limited"].any()
        t.limiter_reset(1)
        assert t.L.tlb_tick_limiter_reset(t.h, ns) == 18
    else:
        assert t.L.tlb_tick_limiter_reset(t.h, -1) == 18 and t.L.tlb_tick_enable_limiter(t.h, None) == 18      # off; and not after the first submit
    t.close()


def test_node_limiter(M, tick_in, chains):
    """two shards on the one GPU: records by node-wide index equal the batch-plane chain's; with the fault-injection build present, a
    broken shard's streams answer NULL while the others carry on, and a restarted shard is enabled again with the same parameters, from
    zero; a BATCH node refuses"""
    cfgs, inter = tick_in
    _, _, recs = chains[True]
    ns = len(cfgs)
    fi = M.load_fault_library() if M.FAULT_LIB_PATH.exists() else None
    nd = M.Node(LM.LL.stream_configs(cfgs), devices=(0, 0), plane="tick", egress="frames", lib=fi)
    assert nd.limiter(0) is None
    nd.enable_limiter(0, 20)
    nd.enable_limiter(M.TRUEPEAK_CEILING_DEFAULT, 20)                # the same parameters, the default named
    with pytest.raises(M.ToolameError) as err:
        nd.enable_limiter(0, 21)
    assert err.value.code == 18
    (f1, n1) = nd.blocks[1]
    mine = [s for s in range(ns) if f1 <= s < f1 + n1]
    others = [s for s in range(ns) if s not in mine]
    assert mine and others

    def step(f, check, want):
        nd.set_pcm(inter[f])
        nd.run()
        for s in check:
            assert nd.limiter(s).tobytes() == want[s].tobytes(), (f, s, nd.limiter(s), want[s])

    for f in range(2):
        step(f, range(ns), recs[f])
    if fi is not None:
        nd.fail_next(1, 1)
        nd.set_pcm(inter[2])
        with pytest.raises(M.ToolameError) as err:
            nd.run()
        assert err.value.code == 17 and not nd.shard_ok(1)
        for s in range(ns):
            assert (nd.limiter(s) is None) if s in mine else (nd.limiter(s).tobytes() == recs[2][s].tobytes()), s
        nd.shard_restart(1)
        for s in mine:
            assert nd.limiter(s).tobytes() == bytes(32)              # from zero: its streams are fresh
        # the restarted shard's streams go on as a fresh limiter with the same parameters would, from tick 3 on
        e = LM.LimiterEmu([cfgs[s] for s in mine], 0, 20)
        b = M.Batch(LM.LL.stream_configs(cfgs))
        for f in range(3, T):
            planar, _ = b.ingest(inter[f:f + 1])
            _, want = e.limit(planar[:, mine])
            nd.set_pcm(inter[f])
            nd.run()
            for k, s in enumerate(mine):
                assert nd.limiter(s).tobytes() == want[k].tobytes(), (f, s)
            for s in others:
                assert nd.limiter(s).tobytes() == recs[f][s].tobytes(), (f, s)
        b.close()
        assert int(nd.limiter(mine[0])["frames"]) == T - 3 and int(nd.limiter(others[0])["frames"]) == T
    else:
        for f in range(2, T):
            step(f, range(ns), recs[f])
    nd.limiter_reset(others[0])
    nd.close()
    b = M.Node(LM.LL.stream_configs(cfgs), devices=(0, 0), plane="batch")
    assert b.L.tlb_node_enable_limiter(b.h, None) == 18 and b.limiter(0) is None and b.L.tlb_node_limiter_reset(b.h, 0) == 18
    b.close()


def test_true_peak_meter_beside_the_limiter_counts_no_over_on_the_burst(M):
    """the 1 kHz burst from -21 dBFS to 0 dBFS through a tick object with both on at the same ceiling: the meter, which sees the limited
    PCM, counts no over; without the limiter it counts the loud half's frames"""
    x = LM.burst()
    cfgs = [dict(samplerate=48000, mode="m")]
    fr = LM.frames_of(x)
    overs = {}
    for on in (False, True):
        t = M.Tick(LM.LL.stream_configs(cfgs), egress="frames")
        if on:
            t.enable_limiter()
        t.enable_truepeak()
        for f in range(fr.shape[0]):
            t.pcm[:] = 0
            t.pcm[0, :N] = fr[f]
            t.run()
        overs[on] = int(t.truepeak["overs"][0])
        if on:
            assert int(t.limiter["limited"][0]) >= 2 and int(t.limiter["peak_in_max"][0]) > M.TRUEPEAK_CEILING_DEFAULT
        t.close()
    assert overs[False] >= 2 and overs[True] == 0, overs
