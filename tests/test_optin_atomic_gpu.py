"""Every opt-in of a tick object is all or nothing (csrc/tlb_mem.h: stage, settle, commit, flag).  The fault-injection build refuses the nth
allocation of the library's memory owner (tlb_debug_alloc_fail_next, csrc/tlb_debug.h): an allocation returns an error code, nothing is
launched.  For enable_short_reads, enable_monitor(AUDIO), enable_compare after it, set_source(stream 0, 44100), enable_loudness and
enable_truepeak the call is made with nth = 1, 2, ... armed until it is accepted: every refused attempt answers TLB_ERR_HIP, leaves the option off and the object healthy, and
the object then produces, tick by tick and at the finish, the bytes of a twin that opted in with nothing armed.  That some attempt was
refused after the first group's buffers had been staged is shown by counting: the same streams as ONE group are refused fewer times.
(A tick object has no tlb_resample_source of its own: "no source" is tlb_tick_need == 1152 here, and 0 from the group's batch is what
that rests on.)  Then the first tlb_decode_device of a batch, and the teardown of an object whose opt-in was refused."""
import numpy as np
import pytest

from pcmgen import gen_pcm

pytestmark = pytest.mark.gpu
HIP, CAP, NT = 17, 64, 4
AUDIO = 2                                                            # TLB_MONITOR_AUDIO
SAMPLES = 1152


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def FI(M):
    lib = M.load_fault_library()
    yield lib
    lib.tlb_debug_alloc_fail_next(0)


def _cfgs(M):
    return [M.StreamConfig(mode="j", bitrate=128, psy_model=1)] * 3 + [M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1)]


@pytest.fixture(scope="module")
def pcm():
    """interleaved int16 [NT][4 streams][2304], seeded; shared and read-only"""
    a = np.stack([np.stack([gen_pcm(40 + s, 0, 0, NT)[f].T.reshape(-1) for s in range(4)]) for f in range(NT)])
    a.setflags(write=False)
    return a


def _tick(M, lib, ngroups=2):
    return M.Tick(_cfgs(M), egress="af", ngroups=ngroups, lib=lib)


def _until_accepted(FI, t, call, is_off):
    """arm nth = 1, 2, ... and make the call until it returns 0 -> the number of refused attempts"""
    refused = 0
    try:
        for nth in range(1, CAP + 1):
            assert FI.tlb_debug_alloc_fail_next(nth) == 0
            rc = call(t)
            if rc == 0:
                return refused
            assert rc == HIP, (nth, rc)
            assert is_off(t), nth
            assert t.status() == 0, nth
            refused += 1
        pytest.fail("not accepted with nth = %d armed" % CAP)
    finally:
        FI.tlb_debug_alloc_fail_next(0)


def _play(t, pcm, before_run, records):
    """NT ticks and the finish -> per step (every stream's packets, the option's records as bytes)"""
    out = []
    for f in range(NT + 1):
        if f < NT:
            t.pcm[:] = pcm[f]
            before_run(t, f)
            t.run()
        else:
            t.finish()
        out.append(([t.packets(s) for s in range(t.nstreams)], records(t)))
    return out


def _short_touch(t, f):
    if f == 2:
        t.valid[1] = 700                                             # one short read, so that the counters move


OPTINS = {
    "short_reads": dict(before=[], call=lambda t: t.L.tlb_tick_enable_short_reads(t.h), off=lambda t: t.valid is None and t.underruns is None,
                        touch=_short_touch, records=lambda t: t.underrun_ms.tobytes() + t.underruns.tobytes()),
    "monitor": dict(before=[], call=lambda t: t.L.tlb_tick_enable_monitor(t.h, AUDIO), off=lambda t: t.monitor is None,
                    touch=lambda t, f: None, records=lambda t: t.monitor.tobytes()),
    "compare": dict(before=[lambda t: t.enable_monitor("audio")], call=lambda t: t.L.tlb_tick_enable_compare(t.h, t.cpar.ctypes.data),
                    off=lambda t: t.compare is None, touch=lambda t, f: None, records=lambda t: t.monitor.tobytes() + t.compare.tobytes()),
    "set_source": dict(before=[], call=lambda t: t.L.tlb_tick_set_source(t.h, 0, 44100), off=lambda t: t.need(0) == SAMPLES,
                       touch=lambda t, f: None, records=lambda t: bytes([t.need(0) & 255, t.need(0) >> 8])),
    # (a batch's meter state that an earlier attempt made stays with the batch; the object's option is off until the whole call goes through)
    "loudness": dict(before=[], call=lambda t: t.L.tlb_tick_enable_loudness(t.h), off=lambda t: t.loudness is None,
                     touch=lambda t, f: None, records=lambda t: t.loudness.tobytes()),
    "truepeak": dict(before=[], call=lambda t: t.L.tlb_tick_enable_truepeak(t.h, 0), off=lambda t: t.truepeak is None,
                     touch=lambda t, f: None, records=lambda t: t.truepeak.tobytes()),
}


@pytest.mark.parametrize("name", list(OPTINS))
def test_a_refused_opt_in_leaves_nothing_and_the_accepted_one_equals_the_twin(M, FI, pcm, name):
    o = OPTINS[name]
    refused = {}
    ticks = {}
    try:
        for ng in (1, 2, 0):                                         # one group (for the count), two groups, the twin (two groups, nothing armed)
            t = _tick(M, FI, ngroups=ng or 2)
            t.cpar = M.compare_params(None)
            for pre in o["before"]:
                pre(t)
            assert o["off"](t)
            if ng:
                refused[ng] = _until_accepted(FI, t, o["call"], o["off"])
            else:
                assert o["call"](t) == 0
            assert not o["off"](t)
            if ng != 1:
                ticks[ng] = _play(t, pcm, o["touch"], o["records"])
            t.close()
    finally:
        FI.tlb_debug_alloc_fail_next(0)
    print("%s: refused %d times as one group, %d times as two" % (name, refused[1], refused[2]))
    assert refused[1] >= 1
    assert refused[2] > refused[1]                                   # some attempt was refused in the second group, behind the first group's staged buffers
    for f in range(NT + 1):
        assert ticks[2][f][0] == ticks[0][f][0], (name, f)
        assert ticks[2][f][1] == ticks[0][f][1], (name, f)
    assert any(p for p in ticks[2][NT][0])                           # (the finish did hand out packets)
    if name == "short_reads":
        assert ticks[2][NT][1] != ticks[2][0][1]                     # (the counters did move)


def test_the_first_decode_of_a_batch_is_refused_whole(M, FI):
    from test_decode_gpu import Hip
    cfgs = _cfgs(M)[2:]
    nf, ns = 2, len(cfgs)
    pcm = np.stack([gen_pcm(60 + s, 0, 0, nf + 1) for s in range(ns)], axis=1)
    b, fresh = M.Batch(cfgs, lib=FI), M.Batch(cfgs, lib=FI)
    out = np.zeros((nf + 1, ns, b.out_stride), dtype=np.uint8)
    lens = np.zeros((nf + 1, ns), dtype=np.int32)
    assert b.L.tlb_encode_host_len(b.h, pcm.ctypes.data, nf + 1, None, None, out.ctypes.data, lens.ctypes.data, None) == 0
    frames, flen = out[1:], lens[1:]                                 # (slot 0 of a first call holds no frame)
    assert (flen > 0).all()
    H = Hip()
    d_fr, d_len, d_rep = H.alloc(frames.nbytes), H.alloc(flen.nbytes), H.alloc(nf * ns * M.FRAME_REPORT_DTYPE.itemsize)
    H.put(d_fr, frames)
    H.put(d_len, flen)
    refused = 0
    try:
        for nth in range(1, CAP + 1):
            assert FI.tlb_debug_alloc_fail_next(nth) == 0
            rc = b.L.tlb_decode_device(b.h, d_fr, d_len, nf, d_rep, None, None, None)
            if rc == 0:
                break
            assert rc == HIP, (nth, rc)
            assert b.decode_bad_frames() == 0
            refused += 1
        else:
            pytest.fail("not accepted with nth = %d armed" % CAP)
    finally:
        FI.tlb_debug_alloc_fail_next(0)
    assert refused >= 1
    got = H.get(d_rep, (nf, ns), M.FRAME_REPORT_DTYPE)
    want, _, _ = fresh.decode(frames, flen)
    assert got.tobytes() == want.tobytes() and not (got["status"] & M.DEC_BAD_MASK).any()
    H.free()
    b.close()
    fresh.close()


def test_an_object_whose_opt_in_was_refused_is_destroyed_cleanly(M, FI, pcm):
    t = _tick(M, FI)
    try:
        assert FI.tlb_debug_alloc_fail_next(1) == 0
        assert t.L.tlb_tick_enable_monitor(t.h, AUDIO) == HIP
    finally:
        FI.tlb_debug_alloc_fail_next(0)
    assert t.monitor is None and t.status() == 0
    t.close()
    t = _tick(M, FI)
    t.pcm[:] = pcm[0]
    t.run()
    t.pcm[:] = pcm[1]
    t.run()
    assert t.status() == 0 and all(len(t.packets(s)) == t.units[s] for s in range(t.nstreams))
    t.close()
