"""The loudness range on the GPU (csrc/toolame_loudness.hip: tl_lra_kernel, tl_lra_range_kernel; tlb_lra_* / tlb_tick_*lra* /
tlb_node_*lra*): the device against the emulation of tests/lralib.py bit for bit on the 37-stream, 230-frame case in three cuts -- range
records, and loudness records with and without the range -- the life-cycle calls and the enable order; a tick object with the range against
one with loudness alone (byte-identical packets and loudness records) and against the emulation, in both loops with 1 and 2 groups; the
node level with a restarted shard; and a batch that never enables the range allocating nothing new."""
import ctypes as C

import numpy as np
import pytest

import loudnesslib as LL
import lralib as RL

pytestmark = pytest.mark.gpu
S = RL.STREAMS
NS = len(S)
N = RL.N


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def pcm():
    return RL.pcm_of(S, RL.NFRAMES)


@pytest.fixture(scope="module")
def emu(pcm):
    """the emulation over the whole signal, once: loudness records after every frame (run frame by frame: the CPU tests show that the cut
    does not matter), range records and programme at the end"""
    e = RL.LraEmu(S)
    recs = {}
    for f in range(RL.NFRAMES):
        recs[f + 1] = e.loudness(pcm[f:f + 1])
    return recs, e.lra(), e.programme()


def _same(got, want):
    assert got.dtype.itemsize == want.dtype.itemsize and got.dtype.names == want.dtype.names
    return got.tobytes() == want.tobytes()


def test_the_shape_is_the_one_the_kernel_can_get_wrong(emu):
    recs, lra, _ = emu
    assert NS == 37 and RL.NFRAMES * N // 4800 - 29 == 26
    live = [s for s in range(NS) if s not in (RL.SILENT, RL.QUIET)]
    assert [int(lra["blocks"][s]) for s in live] == [RL.NFRAMES * N // (S[s]["samplerate"] // 10) - 29 for s in live]
    assert lra[RL.SILENT].tobytes() == bytes(40) and lra[RL.QUIET].tobytes() == bytes(40) and recs[RL.NFRAMES]["short_term"][RL.QUIET] > 0
    assert lra["low_bin"][RL.CONSTANT] == lra["high_bin"][RL.CONSTANT] > 0 and lra["gated"][RL.CONSTANT] == lra["blocks"][RL.CONSTANT]
    stairs = [s for s in live if s != RL.CONSTANT]
    assert (lra["high_bin"][stairs] > lra["low_bin"][stairs]).all()   # r_lo != r_hi and the staircases spread


@pytest.mark.parametrize("cuts", RL.CUTS, ids=["one", "frames", "7+223"])
def test_device_equals_emulation(M, pcm, emu, cuts):
    recs, lra, prog = emu
    b, p = M.Batch(LL.stream_configs(S)), M.Batch(LL.stream_configs(S))      # with the range, and with loudness alone
    for x in (b, p):
        x.enable_loudness()
    b.enable_lra()
    b.enable_lra()                                                   # a second call answers OK
    f0 = 0
    for n in cuts:
        got, plain = b.loudness(pcm[f0:f0 + n]), p.loudness(pcm[f0:f0 + n])
        f0 += n
        assert _same(got, recs[f0]), (cuts, f0, [s for s in range(NS) if got[s].tobytes() != recs[f0][s].tobytes()][:6])
        assert _same(plain, recs[f0]), (cuts, f0)
    got = b.lra()
    assert _same(got, lra), [(s, got[s], lra[s]) for s in range(NS) if got[s].tobytes() != lra[s].tobytes()][:4]
    assert _same(b.loudness_programme(), prog) and _same(p.loudness_programme(), prog)
    assert [M.lra_lu(got[s]) for s in range(NS)] == [RL.lu(lra[s]) for s in range(NS)]
    assert M.LRA_DTYPE.itemsize == 40
    b.close(); p.close()


def test_life_cycle_and_enable_order(M, pcm):
    """refused before loudness is on; loudness_reset of one stream, tlb_stream_reset, tlb_stream_reconfigure to another rate and channel
    count zero the stream's range counts, tlb_stream_finish leaves them; bad arguments change nothing"""
    new = dict(samplerate=16000, mode="m")
    b, e = M.Batch(LL.stream_configs(S)), RL.LraEmu(S)
    rec = np.zeros(NS, dtype=M.LRA_DTYPE)
    assert b.L.tlb_lra_enable(b.h) == 18 and b.L.tlb_lra_host(b.h, rec.ctypes.data) == 18      # loudness first
    b.enable_loudness()
    assert b.L.tlb_lra_host(b.h, rec.ctypes.data) == 18 and b.L.tlb_lra_device(b.h, 64, None) == 18      # never enabled
    b.enable_lra()
    assert b.L.tlb_lra_host(b.h, None) == 18 and b.L.tlb_lra_device(b.h, 64 + 4, None) == 18      # a misaligned device pointer is refused before it is used
    assert not rec.view(np.uint8).any()
    assert _same(b.loudness(pcm[:120]), e.loudness(pcm[:120]))
    before = b.lra()
    assert _same(before, e.lra()) and all(before["blocks"][s] > 0 for s in (3, 4, 8, 9))      # (stream 5 is the silent one)
    b.loudness_reset(3); e.reset(3)
    b.stream_reset(4); e.reset(4)
    b.stream_reconfigure(8, LL.stream_configs([new])[0]); e.reconfigure(8, new)
    b.stream_finish(9)
    mid = b.lra()
    assert _same(mid, e.lra())
    assert [int(mid["blocks"][s]) for s in (3, 4, 8)] == [0, 0, 0] and mid[9].tobytes() == before[9].tobytes()
    assert _same(b.loudness(pcm[120:175]), e.loudness(pcm[120:175]))
    got = b.lra()
    assert _same(got, e.lra())
    assert int(got["blocks"][8]) == 55 * N // 1600 - 29 and int(got["blocks"][10]) == 175 * N // (S[10]["samplerate"] // 10) - 29
    b.loudness_reset(); e.reset(-1)
    assert not b.lra().view(np.uint8).any()
    assert _same(b.loudness(pcm[175:176]), e.loudness(pcm[175:176]))
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
TS = S[:13]                                                          # the tick and node cases: every rate twice, one and two channels
T = 70                                                               # 80 640 samples: 50 bins at 16 kHz (the silent and the quiet stream), 36 at 22.05 kHz, 33 at 24 kHz: range blocks on four streams


@pytest.fixture(scope="module")
def tick_in(M):
    """what the caller hands in, int16 [T][ns][2304] interleaved (a one-channel stream is its first 1152 values), and the planar PCM the
    ingest makes of it, which is what the meter is defined on.  The staircases step every 23 frames: three levels"""
    planar = RL.pcm_of(TS, T)
    inter = np.zeros((T, len(TS), 2 * N), dtype=np.int16)
    for s, c in enumerate(TS):
        if LL.nch_of(c) == 2:
            inter[:, s] = planar[:, s].transpose(0, 2, 1).reshape(T, -1)
        else:
            inter[:, s, :N] = planar[:, s, 0]
            inter[:, s, N:] = 0x1234
    b = M.Batch(LL.stream_configs(TS))
    got, _ = b.ingest(inter)
    b.close()
    for s, c in enumerate(TS):
        assert np.array_equal(got[:, s, :LL.nch_of(c)], planar[:, s, :LL.nch_of(c)]), s
    return inter, got


@pytest.fixture(scope="module")
def tick_emu(tick_in):
    e = RL.LraEmu(TS)
    recs = [e.loudness(tick_in[1][f:f + 1]) for f in range(T)]
    lra = e.lra()
    assert (lra["blocks"] > 0).sum() >= 4 and (lra["high_bin"] > lra["low_bin"]).any()
    return recs, lra, e.programme()


def _loop(t, inter, pipelined, after):
    """the ticks of `inter` in either loop -- run(), or submit, submit, wait ... -- then finish; after(i) follows every wait"""
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


@pytest.mark.parametrize("ngroups,pipelined", [(1, False), (2, True), (2, False), (1, True)])
def test_tick_with_lra_against_one_without_and_against_the_emulation(M, tick_in, tick_emu, ngroups, pipelined):
    """packets and loudness records byte for byte against a tick with loudness alone, and both against the emulation after every wait;
    Tick.lra() equals the emulation at the end"""
    inter, _ = tick_in
    recs, lra, prog = tick_emu
    cfgs, ns = LL.stream_configs(TS), len(TS)
    snaps = []
    for on in (False, True):
        t = M.Tick(cfgs, egress="frames", ngroups=ngroups)
        rec = np.zeros(ns, dtype=M.LRA_DTYPE)
        if on:
            assert t.L.tlb_tick_enable_lra(t.h) == 18                # loudness first
        t.enable_loudness()
        if on:
            t.enable_lra()
            t.enable_lra()
            assert not t.lra().view(np.uint8).any()
        else:
            assert t.L.tlb_tick_lra(t.h, rec.ctypes.data) == 18
        got = []

        def after(i):
            got.append([(t.frame(s), tuple(int(x) for x in t.peaks[s])) for s in range(ns)])
            assert _same(t.loudness, recs[i]), (on, i)

        _loop(t, inter, pipelined, after)
        if on:
            assert _same(t.lra(), lra)
        assert _same(t.loudness_programme(), prog)
        t.close()
        snaps.append(got)
    assert len(snaps[0]) == T and all(len(x[0]) > 0 for x in snaps[0][1])
    assert snaps[1] == snaps[0]


def test_tick_enable_is_refused_after_the_first_submit_and_with_a_tick_in_flight(M, tick_in):
    inter, _ = tick_in
    t = M.Tick(LL.stream_configs(TS[:4]), egress="frames")
    t.enable_loudness()
    t.pcm[:] = inter[0, :4]
    t.run()
    rec = np.zeros(4, dtype=M.LRA_DTYPE)
    assert t.L.tlb_tick_enable_lra(t.h) == 18 and t.L.tlb_tick_lra(t.h, rec.ctypes.data) == 18      # after the first submit; never enabled
    t.close()
    t = M.Tick(LL.stream_configs(TS[:4]), egress="frames")
    t.enable_loudness()
    t.enable_lra()
    t.pcm[:] = inter[0, :4]
    t.submit()
    assert t.L.tlb_tick_lra(t.h, rec.ctypes.data) == 18              # a tick is in flight
    t.wait()
    assert t.L.tlb_tick_enable_lra(t.h) == 18                        # the opt-in calls are for before the first submit, even when already on
    assert t.L.tlb_tick_lra(t.h, None) == 18
    t.lra()
    t.close()


def test_node_lra(M, tick_in, tick_emu):
    """two shards on the one GPU: Node.lra() equals the emulation's; with the fault-injection build present, a broken shard's block is all
    zero while the other carries on, and a restarted shard is enabled again and counts from zero; a BATCH node refuses"""
    inter, planar = tick_in
    ns = len(TS)
    fi = M.load_fault_library() if M.FAULT_LIB_PATH.exists() else None
    nd = M.Node(LL.stream_configs(TS), devices=(0, 0), plane="tick", egress="frames", ngroups=2, lib=fi)
    e = RL.LraEmu(TS)
    rec = np.zeros(ns, dtype=M.LRA_DTYPE)
    assert nd.L.tlb_node_enable_lra(nd.h) == 18 and nd.L.tlb_node_lra(nd.h, rec.ctypes.data) == 18      # loudness first
    nd.enable_loudness()
    nd.enable_lra()
    nd.enable_lra()
    (f1, n1) = nd.blocks[1]
    mine = [s for s in range(ns) if f1 <= s < f1 + n1]
    others = [s for s in range(ns) if s not in mine]
    assert mine and others

    def steps(f0, f1_, check):
        for f in range(f0, f1_):
            nd.set_pcm(inter[f])
            nd.run()
            want = e.loudness(planar[f:f + 1])
        for s in check:
            assert nd.loudness(s).tobytes() == want[s].tobytes(), (f1_, s)

    steps(0, 62, range(ns))                                          # 32 bins at 22.05 kHz: the first range blocks exist
    got = nd.lra()
    assert _same(got, e.lra()) and (got["blocks"] > 0).any()
    if fi is not None:
        nd.fail_next(1, 1)
        nd.set_pcm(inter[62])
        with pytest.raises(M.ToolameError) as err:
            nd.run()
        assert err.value.code == 17 and not nd.shard_ok(1)
        e.loudness(planar[62:63])
        got, want = nd.lra(), e.lra()
        assert not got[mine].view(np.uint8).any() and got[others].tobytes() == want[others].tobytes()
        nd.shard_restart(1)
        for s in mine:
            e.reset(s)
        assert not nd.lra()[mine].view(np.uint8).any()
        steps(63, T, range(ns))
    else:
        steps(62, T, range(ns))
    got = nd.lra()
    assert _same(got, e.lra()) and (got["blocks"][others] > 0).any()
    nd.close()
    b = M.Node(LL.stream_configs(TS), devices=(0, 0), plane="batch")
    assert b.L.tlb_node_enable_lra(b.h) == 18 and b.L.tlb_node_lra(b.h, rec.ctypes.data) == 18
    b.close()


def _free_bytes(M):
    """free device memory as the HIP runtime the library is linked against reports it"""
    M.load_library()
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = C.CDLL(path)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_a_batch_that_never_enables_the_range_allocates_nothing_new(M):
    """4096 streams, so that the range's 3008 bytes per stream (12.3 MB) cannot hide in the allocator's granularity: with loudness alone,
    measuring, the programme and the life-cycle calls leave the free device memory where it was; tlb_lra_enable then takes the counts and
    the records' scratch, and no more than 2 MiB of rounding beside them"""
    ns = 4096
    cfgs = [dict(samplerate=LL.RATES[s % 6], mode="m" if (s // 6 + s) % 2 else "s") for s in range(ns)]
    pcm = np.zeros((1, ns, 2, N), dtype=np.int16)
    b = M.Batch(LL.stream_configs(cfgs))
    b.enable_loudness()
    b.loudness(pcm); b.loudness_programme(); b.stream_reset(1)       # once ahead of the first reading: whatever the first call of a kind takes
    free0 = _free_bytes(M)
    b.loudness(pcm); b.loudness_programme(); b.loudness_reset(0); b.stream_reset(1); b.stream_finish(2)
    free1 = _free_bytes(M)
    assert free1 == free0
    b.enable_lra()
    free2 = _free_bytes(M)
    b.enable_lra()
    assert _free_bytes(M) == free2
    assert ns * 3008 <= free1 - free2 <= ns * (3008 + 40) + (2 << 20), free1 - free2
    b.loudness(pcm)
    assert not b.lra().view(np.uint8).any() and _free_bytes(M) == free2
    b.close()
