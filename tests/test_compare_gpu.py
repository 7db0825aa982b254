"""The compare monitor on the GPU (csrc/toolame_compare.hip, tlb_compare_* / tlb_tick_*compare* / tlb_node_*compare*).  The oracle is the
plain Python-int loop of tests/comparelib.py over what a SEPARATE Batch.decode says about the frames the caller received: batch level
(one call, ragged cuts, the flush, exchanged / swapped / zeroed decoded PCM, a stream reset, the argument errors), a tick object after
every wait against one that never enabled it, an exchange of two input rows, the enable ordering, and the node level."""
import ctypes as C

import numpy as np
import pytest

import comparelib as CL

pytestmark = pytest.mark.gpu
NF = 6
NCH = [CL.nch_of(c) for c in CL.STREAMS]
NS = len(NCH)
P = CL.PARAMS
ARG = 18


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def _cfgs(M):
    return [M.StreamConfig(samplerate=c["samplerate"], mode=c["mode"], bitrate=c["kbps"], psy_model=1) for c in CL.STREAMS]


@pytest.fixture(scope="module")
def run(M):
    """the shared run on the device: pcm [NF], frames / reports / decoded PCM [NF + 1] (the last slot is the flush), the oracle's records"""
    pcm = CL.noise(NF, NS)
    b = M.Batch(_cfgs(M))
    out = np.zeros((NF + 1, NS, b.out_stride), dtype=np.uint8)
    lens = np.zeros((NF + 1, NS), dtype=np.int32)
    assert b.L.tlb_encode_host_len(b.h, pcm.ctypes.data, NF, None, None, out.ctypes.data, lens.ctypes.data, None) == 0
    assert b.L.tlb_flush_host_len(b.h, out[NF].ctypes.data, lens[NF].ctypes.data) == 0
    rep, _, dec = b.decode(out, lens, want_pcm=True)
    st = rep["status"].astype(int)
    assert (st[0] == M.DEC_EMPTY).all() and not (st[1:] & (M.DEC_EMPTY | M.DEC_BAD_MASK)).any()
    o = CL.Oracle(NCH)
    want, seen = o.compare(pcm, dec[:NF], st[:NF], P)
    want_f, seen_f = o.compare(None, dec[NF:], st[NF:], P, want)
    CL.check_input_conditions(seen + seen_f, CL.mispaired_sums(pcm, dec[:NF], NCH), set(range(NS)))
    assert (want_f["frames_judged"] == NF).all() and (want_f["frames_compared"] == NF).all() and not want_f["mismatch_frames"].any()
    for a in (pcm, rep, dec, want, want_f):
        a.setflags(write=False)
    yield dict(b=b, pcm=pcm, rep=rep, dec=dec, st=st, want=want, want_f=want_f)
    b.close()


def test_one_call_ragged_cuts_and_the_flush_equal_the_oracle(M, run):
    b = run["b"]
    b.compare_reset()
    rec = b.compare(run["pcm"], run["dec"][:NF], run["rep"][:NF], P)
    assert rec.dtype == M.COMPARE_DTYPE == CL.RECORD_DTYPE
    CL.same(rec, run["want"], "one call")
    b.compare(None, run["dec"][NF:], run["rep"][NF:], P, rec)
    CL.same(rec, run["want_f"], "flush")
    b.compare(None, run["dec"][NF:], run["rep"][NF:], P, rec)        # the flush does not advance the history: the same sums again
    assert rec["sxy"].tolist() == run["want_f"]["sxy"].tolist() and (rec["frames_compared"] == NF + 1).all()
    b.compare_reset()
    rec = np.zeros(NS, dtype=M.COMPARE_DTYPE)
    pos = 0
    for cut in (1, 3, 2):
        assert b.compare(run["pcm"][pos:pos + cut], run["dec"][pos:pos + cut], run["rep"][pos:pos + cut], P, rec) is rec
        pos += cut
    CL.same(rec, run["want"], "1 + 3 + 2")
    b.compare(None, run["dec"][NF:], run["rep"][NF:], P, rec)
    CL.same(rec, run["want_f"], "1 + 3 + 2 + flush")


def test_exchanged_swapped_and_zeroed_decodes_equal_the_oracle(M, run):
    """the mono pair's decoded PCM exchanged, the stereo stream's channels exchanged, the dual-channel stream's decode zeroed -- in one call"""
    b = run["b"]
    dec = run["dec"][:NF].copy()
    dec[:, [3, 4]] = dec[:, [4, 3]]
    dec[:, 0] = dec[:, 0, ::-1]
    dec[:, 2] = 0
    want, _ = CL.Oracle(NCH).compare(run["pcm"], dec, run["st"][:NF], P)
    assert list(want["mismatch_frames"]) == [NF - 1, 0, NF - 1, NF - 1, NF - 1, 0] and list(want["swapped_frames"]) == [NF - 1, 0, 0, 0, 0, 0]
    b.compare_reset()
    rec = b.compare(run["pcm"], dec, run["rep"][:NF], P)
    CL.same(rec, want)
    for s in (1, 5):                                                 # every other record equals the undisturbed run
        assert rec[s].tobytes() == run["want"][s].tobytes()


def test_a_bad_slot_and_a_stream_reset(M, run):
    """a BAD report is skipped and the next slot aligns; tlb_stream_reset between two calls clears that stream's history and no other's"""
    b = run["b"]
    rep, dec = run["rep"][:NF].copy(), run["dec"][:NF].copy()
    rep["status"][3, 1] |= M.DEC_BAD_MASK & 0x08
    dec[3, 1] = 0
    o = CL.Oracle(NCH)
    want, _ = o.compare(run["pcm"][:3], dec[:3], rep["status"][:3], P)
    b.compare_reset()
    rec = b.compare(run["pcm"][:3], dec[:3], rep[:3], P)
    CL.same(rec, want, "before the reset")
    b.stream_reset(0)
    o.reset(0)
    want, _ = o.compare(run["pcm"][3:], dec[3:], rep["status"][3:], P, want)
    b.compare(run["pcm"][3:], dec[3:], rep[3:], P, rec)
    CL.same(rec, want, "after the reset")
    assert rec["frames_compared"][1] == NF - 2 and not rec["mismatch_frames"].any() and rec["frames_judged"][0] == NF - 2
    assert rec["sxy"][1].tolist() == run["want"]["sxy"][1].tolist()


def test_argument_errors_change_nothing(M, run):
    b, L = run["b"], run["b"].L
    rec = np.zeros(NS, dtype=M.COMPARE_DTYPE)
    rec["frames_compared"] = 7
    before = rec.copy()
    pcm, dec, rep = run["pcm"], run["dec"], run["rep"]
    par = M.compare_params(P)
    args = lambda **k: [k.get("b", b.h), k.get("i", pcm.ctypes.data), k.get("d", dec.ctypes.data), k.get("r", rep.ctypes.data), k.get("n", 1),
                        k.get("p", par.ctypes.data), k.get("rec", rec.ctypes.data)]
    for bad in (dict(d=None), dict(r=None), dict(p=None), dict(rec=None), dict(n=0), dict(n=-2), dict(i=None, n=2), dict(i=pcm.ctypes.data + 1),
                dict(rec=rec.ctypes.data + 4)):
        assert L.tlb_compare_host(*args(**bad)) == ARG, bad
    for params in ((0, 1, 2), (P[0], 0, 2), (P[0], 3, 2), (P[0], 1, 1025), (P[0], -1, 2)):
        assert L.tlb_compare_host(*args(p=M.compare_params(params).ctypes.data)) == ARG, params
    dv = lambda a: C.c_void_p(a)
    assert L.tlb_compare_device(b.h, dv(4096), dv(4096 + 8), dv(4096), 1, par.ctypes.data, dv(4096), None) == ARG       # PCM moves in 16-byte pieces
    assert L.tlb_compare_device(b.h, dv(4096 + 2), dv(4096), dv(4096), 1, par.ctypes.data, dv(4096), None) == ARG
    assert L.tlb_compare_device(b.h, dv(4096), dv(4096), dv(4096 + 2), 1, par.ctypes.data, dv(4096), None) == ARG
    assert L.tlb_compare_device(b.h, dv(4096), dv(4096), None, 1, par.ctypes.data, dv(4096), None) == ARG
    assert L.tlb_compare_reset(b.h, NS) == ARG and L.tlb_compare_reset(b.h, -2) == ARG
    assert rec.tobytes() == before.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
def _received(t, bd):
    """the frames the caller received this tick as one slot of a separate batch's decode input"""
    fr = np.zeros((1, NS, bd.out_stride), dtype=np.uint8)
    ln = np.zeros((1, NS), dtype=np.int32)
    raw = []
    for s in range(NS):
        f = t.frame(s)
        raw.append(f)
        fr[0, s, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        ln[0, s] = len(f)
    return fr, ln, raw


def test_tick_records_equal_the_loop_after_every_tick(M, run):
    """two groups, six ticks and the finish: after every tick Tick.compare equals the Python loop over a separate Batch.decode of the frames
    the caller received; a tick object that never enabled it has no accessor and hands out the same bytes"""
    inter = CL.interleaved_of(run["pcm"], NCH)
    t = M.Tick(_cfgs(M), egress="frames", ngroups=2)
    plain = M.Tick(_cfgs(M), egress="frames", ngroups=2)
    bd = M.Batch(_cfgs(M))
    t.enable_monitor("audio")
    assert t.compare is None
    t.enable_compare(P)
    assert plain.compare is None
    o = CL.Oracle(NCH)
    want = np.zeros(NS, dtype=CL.RECORD_DTYPE)
    for f in range(NF + 1):
        if f < NF:
            t.pcm[:] = inter[f]
            plain.pcm[:] = inter[f]
            t.run()
            plain.run()
        else:
            t.finish()
            plain.finish()
        fr, ln, raw = _received(t, bd)
        assert raw == [plain.frame(s) for s in range(NS)], f
        assert (ln[0] > 0).all() == (f > 0)
        rep, _, dec = bd.decode(fr, ln, want_pcm=True)
        want, _ = o.compare(CL.planar_of(inter[f], NCH) if f < NF else None, dec, rep["status"].astype(int), P, want)
        got = t.compare
        assert got is not None and got.dtype == M.COMPARE_DTYPE
        CL.same(got.copy(), want, f)
        assert plain.compare is None
    CL.same(t.compare.copy(), run["want_f"], "the batch-level run")
    assert (t.compare["frames_compared"] == NF).all() and (t.monitor["frames"] == NF).all()
    for x in (t, plain, bd):
        x.close()


def test_tick_with_two_input_rows_exchanged_for_one_tick(M, run):
    """The two streams of the mono pair get each other's row of the pinned PCM in the last tick only.  The object is GIVEN the exchanged
    rows as its input and its own frames carry exactly that audio, so its records equal the loop fed with the rows as they were and count
    no mismatch: the compare sees what lies between the encoder's input and the frame that leaves, not what lies ahead of the input.
    Against the programme each stream was MEANT to carry -- the loop fed with the rows as they should have been -- the fault shows one
    frame later, at the finish, when the frame made of the exchanged rows leaves: both streams' correlation falls out of the healthy range
    (below 0.6 where every other slot is above 3/4).  It does not fall to nothing: 481 of that slot's 1152 samples are still the stream's
    own (the delay), so the figure is 0.42 .. 0.49 (measured: 0.42 and 0.49), too near the 1/2 of the tests' params to assert a count on."""
    inter = CL.interleaved_of(run["pcm"], NCH)
    fed = inter.copy()
    fed[NF - 1, [3, 4]] = inter[NF - 1, [4, 3]]
    t = M.Tick(_cfgs(M), egress="frames", ngroups=2)
    bd = M.Batch(_cfgs(M))
    t.enable_monitor("audio")
    t.enable_compare(P)
    o_fed, o_meant = CL.Oracle(NCH), CL.Oracle(NCH)
    w_fed = np.zeros(NS, dtype=CL.RECORD_DTYPE)
    w_meant = w_fed.copy()
    for f in range(NF + 1):
        if f < NF:
            t.pcm[:] = fed[f]
            t.run()
        else:
            t.finish()
        fr, ln, _ = _received(t, bd)
        rep, _, dec = bd.decode(fr, ln, want_pcm=True)
        st = rep["status"].astype(int)
        w_fed, _ = o_fed.compare(CL.planar_of(fed[f], NCH) if f < NF else None, dec, st, P, w_fed)
        w_meant, seen = o_meant.compare(CL.planar_of(inter[f], NCH) if f < NF else None, dec, st, P, w_meant)
        CL.same(t.compare.copy(), w_fed, f)
        for _, s, sxx, syy, sxy, _ in seen:
            c = CL.corr(sxy[0], sxx[0], syy[0])
            print("tick %d stream %d: correlation with the programme it was meant to carry %.4f" % (f, s, c))
            assert (c < 0.6) if (f == NF and s in (3, 4)) else (c >= 0.75), (f, s, c)
    assert not t.compare["mismatch_frames"].any() and (t.compare["frames_judged"] == NF).all() and (t.compare["frames_compared"] == NF).all()
    t.close()
    bd.close()


def test_tick_counts_the_mismatches_of_two_crossed_slots(M, run):
    """The fault the compare is for, inside a tick object (fault-injection build, csrc/tlb_debug.h): from tick 2 on the frames of the two
    streams of the mono pair leave in each other's slots -- valid frames, the other stream's programme.  The monitor record notices one
    frame (the first crossed frame's ScF-CRC is its own stream's: BAD, skipped by the compare); the compare record counts every frame after
    it: mismatch_frames and mismatch_run grow tick by tick through the tick's record copy-out and reach 3, no other stream moves, and after
    every tick the record equals the loop over a separate decode of the frames the caller received.  The crossed correlation is that of
    two independent programmes (at most 1/4), far from the 1/2 of the params."""
    FI = M.load_fault_library()
    inter = CL.interleaved_of(run["pcm"], NCH)
    t = M.Tick(_cfgs(M), egress="frames", ngroups=2, lib=FI)
    bd = M.Batch(_cfgs(M))
    t.enable_monitor("audio")
    t.enable_compare(P)
    assert FI.tlb_debug_tick_cross_from(t.h, 0, 4, 1) == ARG        # two groups: streams 0 and 4 do not share one
    t.cross_from(3, 4, nth=3)                                        # ticks 0 and 1 healthy
    o = CL.Oracle(NCH)
    want = np.zeros(NS, dtype=CL.RECORD_DTYPE)
    runs = []
    for f in range(NF + 1):
        if f < NF:
            t.pcm[:] = inter[f]
            t.run()
        else:
            t.finish()
        fr, ln, _ = _received(t, bd)
        rep, _, dec = bd.decode(fr, ln, want_pcm=True)
        want, seen = o.compare(CL.planar_of(inter[f], NCH) if f < NF else None, dec, rep["status"].astype(int), P, want)
        got = t.compare.copy()
        CL.same(got, want, f)
        runs.append([int(got["mismatch_run"][s]) for s in (3, 4)])
        for _, s, sxx, syy, sxy, _ in seen:
            c = CL.corr(sxy[0], sxx[0], syy[0])
            assert (abs(c) <= 0.25) if (s in (3, 4) and f >= 3) else (c >= 0.75), (f, s, c)
    assert runs == [[0, 0], [0, 0], [0, 0], [1, 1], [2, 2], [3, 3], [4, 4]]
    got, mon = t.compare, t.monitor
    assert list(got["mismatch_frames"]) == [0, 0, 0, 4, 4, 0] and list(got["frames_compared"]) == [NF, NF, NF, NF - 1, NF - 1, NF]
    assert (got["last_flags"][[3, 4]] == (CL.JUDGED0 | CL.MISMATCH)).all() and not got["swapped_frames"].any()
    assert list(mon["bad_frames"]) == [0, 0, 0, 1, 1, 0] and (mon["frames"] == NF).all()
    for s in (0, 1, 2, 5):
        assert got[s].tobytes() == run["want_f"][s].tobytes()
    t.close()
    bd.close()


def test_every_life_cycle_call_clears_the_history(M):
    """tlb_stream_finish, tlb_stream_reconfigure and tlb_reset, like tlb_stream_reset: the history of the streams they touch is zeros
    afterwards -- the next slot has nothing to be set against -- the others' is kept, and no record moves"""
    cfgs = _cfgs(M)
    b = M.Batch(cfgs)
    pcm = CL.noise(3, NS, seed=2000)
    rep = np.zeros((1, NS), dtype=M.FRAME_REPORT_DTYPE)              # status 0: every slot is compared
    for op, touched in ((lambda: b.stream_finish(1), [1]), (lambda: b.stream_reconfigure(1, cfgs[1]), [1]), (lambda: b.stream_reset(2), [2]),
                        (lambda: b.reset(), list(range(NS))), (lambda: b.compare_reset(4), [4])):
        b.compare_reset()
        o = CL.Oracle(NCH)
        rec = b.compare(pcm[:2], pcm[:2], np.repeat(rep, 2, axis=0), P)       # the history now holds pcm[1] behind the tail of pcm[0]
        want, _ = o.compare(pcm[:2], pcm[:2], np.zeros((2, NS), dtype=int), P)
        before = rec.copy()
        op()
        for s in touched:
            o.reset(s)
        b.compare(pcm[2:], pcm[1:2], rep, P, rec)                    # "decoded": the frame before at no delay, so a kept history correlates a little, a zero one is not judged
        want, seen = o.compare(pcm[2:], pcm[1:2], np.zeros((1, NS), dtype=int), P, want)
        CL.same(rec, want, touched)
        for _, s, sxx, _, _, _ in seen:
            assert (max(sxx) == 0) == (s in touched), (touched, s)
        assert (rec["frames_judged"] - before["frames_judged"] == np.array([0 if s in touched else 1 for s in range(NS)])).all()
    b.close()


def test_enable_ordering(M):
    cfgs = _cfgs(M)
    par = M.compare_params(P)
    t = M.Tick(cfgs, egress="frames")
    L = t.L
    assert L.tlb_tick_enable_compare(t.h, par.ctypes.data) == ARG   # no monitor at all
    t.enable_monitor("check")
    assert L.tlb_tick_enable_compare(t.h, par.ctypes.data) == ARG   # not the audio mode
    assert t.compare is None
    t.close()
    t = M.Tick(cfgs, egress="frames")
    t.enable_monitor("audio")
    assert L.tlb_tick_enable_compare(t.h, None) == ARG and L.tlb_tick_enable_compare(t.h, M.compare_params((0, 1, 2)).ctypes.data) == ARG
    assert L.tlb_tick_enable_compare(t.h, par.ctypes.data) == 0 and L.tlb_tick_enable_compare(t.h, par.ctypes.data) == 0      # identical again: OK
    assert L.tlb_tick_enable_compare(t.h, M.compare_params((P[0], 3, 4)).ctypes.data) == ARG
    assert L.tlb_tick_enable_monitor(t.h, 3) == ARG and L.tlb_tick_enable_monitor(t.h, 4) == ARG
    t.close()
    t = M.Tick(cfgs, egress="frames")
    t.enable_monitor("audio")
    t.pcm[:] = 0
    t.run()
    assert L.tlb_tick_enable_compare(t.h, par.ctypes.data) == ARG   # after the first submit
    assert t.compare is None
    t.close()


def test_node_records_equal_one_tick_object_s(M, run):
    """two shards on one device: the records by node-wide index equal those of one Tick over the same streams, tick by tick; a BATCH-plane
    node refuses"""
    inter = CL.interleaved_of(run["pcm"], NCH)
    nd = M.Node(_cfgs(M), devices=(0, 0), plane="tick", egress="frames")
    t = M.Tick(_cfgs(M), egress="frames")
    par = M.compare_params(P)
    assert nd.L.tlb_node_enable_compare(nd.h, par.ctypes.data) == ARG            # before the audio monitor
    nd.enable_monitor("audio")
    assert nd.compare(0) is None
    nd.enable_compare(P)
    nd.enable_compare(P)
    assert nd.L.tlb_node_enable_compare(nd.h, M.compare_params((P[0], 3, 4)).ctypes.data) == ARG
    t.enable_monitor("audio")
    t.enable_compare(P)
    for f in range(NF + 1):
        if f < NF:
            nd.set_pcm(inter[f])
            t.pcm[:] = inter[f]
            nd.run()
            t.run()
        else:
            nd.finish()
            t.finish()
        one = t.compare
        for s in range(NS):
            got = nd.compare(s)
            assert got is not None and got.tobytes() == one[s].tobytes(), (f, s)
    assert all(nd.compare(s)["frames_compared"] == NF for s in range(NS))
    CL.same(t.compare.copy(), run["want_f"])
    assert nd.compare(NS) is None and nd.compare(-1) is None
    nd.close()
    t.close()
    nb = M.Node(_cfgs(M), devices=(0, 0), plane="batch")
    assert nb.L.tlb_node_enable_compare(nb.h, par.ctypes.data) == ARG and nb.compare(0) is None
    nb.close()
