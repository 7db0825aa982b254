"""The confidence monitor on the GPU (csrc/toolame_monitor.hip, tlb_monitor_* / tlb_tick_*monitor* / tlb_node_*monitor*).  The oracle
of the fold is the plain Python loop of tests/monitorlib.py over what a SEPARATE Batch.decode says about the frames the caller received:
batch level, a tick object with the monitor against one without (byte-identical output), tick against batch after every wait, digital
silence, a stream reset in mid-run, one damaged byte (fault-injection build), listen, the argument errors, and the node level."""
import ctypes as C

import numpy as np
import pytest

import monitorlib as ML
from pcmgen import gen_pcm

pytestmark = pytest.mark.gpu

MIX = [(48000, "s", 128, 1), (48000, "j", 128, 3), (48000, "m", 64, 0), (24000, "m", 64, 1), (44100, "s", 128, 1), (48000, "s", 192, 2),
       (48000, "j", 192, 4), (24000, "j", 64, 1), (48000, "m", 96, 1), (48000, "s", 128, 1), (24000, "s", 64, 1)]
SILENT = (9, 10)                                                     # fed digital silence (psy 1), 48 and 24 kHz
DAB = [s for s in MIX if s[0] != 44100]                              # the AF egress takes whole 24-ms units only
UNCHECKED, EMPTY = 0x20, 0x01


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def FI(M):
    return M.load_fault_library()


def _cfgs(M, streams):
    return [M.StreamConfig(samplerate=r, mode=m, bitrate=k, psy_model=p) for r, m, k, p in streams]


def _rates(streams):
    return [r for r, _, _, _ in streams]


def _inter(streams, T, seed, silent=()):
    ns = len(streams)
    x = np.stack([np.stack([gen_pcm(seed + s, (0, 7, 5, 4)[s % 4], 0, T)[f].T.reshape(-1) for s in range(ns)]) for f in range(T)])      # [T, ns, 2304] L R L R
    for s, (_, m, _, _) in enumerate(streams):
        if m == "m":
            x[:, s, 1152:] = 0x1234                                  # a mono stream is its first 1152 values; the rest is never read
        if s in silent:
            x[:, s] = 0
    return x


def _same(got, want, what=""):
    for k in ML.RECORD_DTYPE.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


# ---------------------------------------------------------------------------------------------------------------------------------
def _encode_slots(M, b, pcm):
    """Batch.encode with the slots kept apart: (out [nf + 1][ns][stride], lens [nf + 1][ns]), the flushed frames as the last slot"""
    nf, ns = pcm.shape[0], b.nstreams
    out = np.zeros((nf + 1, ns, b.out_stride), dtype=np.uint8)
    lens = np.zeros((nf + 1, ns), dtype=np.int32)
    assert b.L.tlb_encode_host_len(b.h, np.ascontiguousarray(pcm).ctypes.data, nf, None, None, out.ctypes.data, lens.ctypes.data, None) == 0
    assert b.L.tlb_flush_host_len(b.h, out[nf].ctypes.data, lens[nf].ctypes.data) == 0
    return out, lens


def test_batch_monitor_equals_the_python_loop(M):
    """a mixed batch (48 kHz s / j / m, 24 kHz, 44.1 kHz, psy 0-4, two silent streams), damaged frames and empty slots: Batch.monitor on the
    output of Batch.decode equals the loop, whole, cut into calls, and without PCM; the argument errors"""
    cfgs, ns, nf = _cfgs(M, MIX), len(MIX), 9
    pcm = np.stack([gen_pcm(9100 + s, 1 if s in SILENT else (0, 7, 5, 4)[s % 4], 0, nf) for s in range(ns)], axis=1)
    b = M.Batch(cfgs)
    frames, lens = _encode_slots(M, b, pcm)
    rng = np.random.default_rng(21)
    for s in (0, 3, 4, 6):                                           # one byte of two frames each: the stored CRC-16, then any byte
        f1, f2 = sorted(rng.choice(np.arange(1, nf + 1), size=2, replace=False))
        frames[f1, s, int(rng.integers(4, 6))] ^= 1 << int(rng.integers(0, 8))
        frames[f2, s, int(rng.integers(0, lens[f2, s]))] ^= 1 << int(rng.integers(0, 8))
    lens[4, 1] = 0; lens[5, 1] = 0; lens[nf, 7] = 0; lens[2, 9] = 0  # empty slots (slot 0 is empty for every stream anyway)
    rep, _, dec = b.decode(frames, lens, want_pcm=True)
    st = rep["status"]
    assert (st[0] == EMPTY).all() and (st[1:, [0, 3, 4, 6]] & M.DEC_BAD_MASK).any(axis=0).all() and not (st[:, [2, 5, 8]] & M.DEC_BAD_MASK).any()
    want = ML.fold_python(st, dec, _rates(MIX))
    _same(b.monitor(rep, dec), want, "whole")
    assert list(want["frames"]) == [nf, nf - 2, nf, nf, nf, nf, nf, nf - 1, nf, nf - 1, nf] and want["bad_frames"].sum() >= 4
    assert (want["out_peak"][[2, 5, 8]] > 0).any(axis=1).all() and not want["out_peak"][3][1] and not want["out_peak"][list(SILENT)].any()
    rec = np.zeros(ns, dtype=M.MONITOR_DTYPE)
    pos = 0
    for cut in (1, 3, 1, 2, nf + 1 - 7):
        assert b.monitor(rep[pos:pos + cut], dec[pos:pos + cut], rec) is rec
        _same(rec, ML.fold_python(st[:pos + cut], dec[:pos + cut], _rates(MIX)), pos)
        pos += cut
    assert pos == nf + 1
    _same(rec, want, "in calls")
    keep = rec.copy()
    b.monitor(rep[1:4], None, rec)                                   # without PCM: counts move, peaks (no empty slot here but stream 9's) and silence stay
    _same(rec, ML.fold_python(st[1:4], None, _rates(MIX), keep), "no pcm")
    assert np.array_equal(rec["out_silence_ms"], keep["out_silence_ms"]) and np.array_equal(rec["out_peak"][:9], keep["out_peak"][:9])
    # argument errors: nothing changes
    L, before = b.L, rec.copy()
    assert L.tlb_monitor_host(b.h, None, None, 1, rec.ctypes.data) == 18 and L.tlb_monitor_host(b.h, rep.ctypes.data, None, 1, None) == 18
    assert L.tlb_monitor_host(b.h, rep.ctypes.data, None, 0, rec.ctypes.data) == 18 and L.tlb_monitor_host(b.h, rep.ctypes.data, None, -3, rec.ctypes.data) == 18
    raw = np.zeros(rec.nbytes + 8, dtype=np.uint8)
    off = (-raw.ctypes.data) % 4 + 2                                 # an address that is 2 mod 4
    assert L.tlb_monitor_host(b.h, rep.ctypes.data, None, 1, raw.ctypes.data + off) == 18
    assert L.tlb_monitor_device(b.h, C.c_void_p(4096 + 2), None, 1, C.c_void_p(4096), None) == 18
    assert L.tlb_monitor_device(b.h, C.c_void_p(4096), C.c_void_p(4096 + 1), 1, C.c_void_p(4096), None) == 18
    assert rec.tobytes() == before.tobytes() and not raw.any()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
class Loop:
    """T ticks of a Tick object in either loop -- run(), or submit, submit, wait ... -- then finish; after every wait (and the finish)
    `after(i)` is called with the 0-based index of the tick whose results the accessors show (T: the flush)."""

    def __init__(self, t, inter, pipelined, before=None):
        self.t, self.inter, self.pipelined, self.before = t, inter, pipelined, before

    def go(self, after):
        t, T = self.t, self.inter.shape[0]
        done = 0
        for f in range(T):
            if self.before:
                self.before(f)
            t.pcm[:] = self.inter[f]
            if not self.pipelined:
                t.run()
                after(f); done += 1
            else:
                t.submit()
                if f >= 1:
                    t.wait()
                    after(done); done += 1
        if self.pipelined:
            t.wait()
            after(done); done += 1
        assert done == T
        t.finish()
        after(T)


@pytest.mark.parametrize("egress,ngroups,pipelined", [("frames", 1, False), ("frames", 3, True), ("af", 3, False), ("af", 1, True)])
def test_tick_output_is_byte_identical_with_and_without_the_monitor(M, egress, ngroups, pipelined):
    streams = MIX if egress == "frames" else DAB
    cfgs, ns, T = _cfgs(M, streams), len(streams), 7
    inter = _inter(streams, T, 9200)
    kw = dict(egress=egress, ngroups=ngroups, version=b"mon", now_s=1712345678, delay_ms=370, tist=True)
    snaps = []
    for what in (None, "audio", "check"):
        t = M.Tick(cfgs, **kw)
        if what:
            t.enable_monitor(what)
        got = []
        Loop(t, inter, pipelined).go(lambda i: got.append([(t.frame(s), t.packets(s), tuple(int(x) for x in t.peaks[s]), int(t.silence_ms[s])) for s in range(ns)]))
        if what:
            assert list(t.monitor["frames"]) == [T] * ns and not t.monitor["bad_frames"].any()
        else:
            assert t.monitor is None
        t.close()
        snaps.append(got)
    assert len(snaps[0]) == T + 1 and all(len(x[0]) > 0 or len(x[1]) > 0 for x in snaps[0][1])
    assert snaps[1] == snaps[0] and snaps[2] == snaps[0]


def _against_batch(M, streams, T, seed, what="audio", ngroups=3, pipelined=False, lib=None, silent=(), damage=None, listen=None, reset=None):
    """A monitored Tick (egress frames) over T ticks + finish.  The frames it hands out go, tick by tick, to a separate Batch.decode of the
    same configurations; after every wait Tick.monitor must equal the Python fold of those reports and PCM up to that tick.
    damage = (stream, byte, xor, tick): armed for that tick's submit.  listen = {tick: stream}: selected before that tick's submit.
    reset = (stream, tick): tlb_tick_stream_reset before that tick's submit.  -> (records after every wait, reports [T + 1][ns])"""
    cfgs, ns = _cfgs(M, streams), len(streams)
    inter = _inter(streams, T, seed, silent)
    t = M.Tick(cfgs, egress="frames", ngroups=ngroups, lib=lib)
    t.enable_monitor(what)
    dec = M.Batch(cfgs)
    rates = _rates(streams)
    want = np.zeros(ns, dtype=ML.RECORD_DTYPE)
    hist, reports, pcms, carried = [], [], [], {}
    state = {"listen": -1}

    def before(f):
        if damage and f == damage[3]:
            t.damage_next(damage[0], damage[1], damage[2], 1)
        if listen and f in listen:
            t.monitor_listen(listen[f])
            state["listen"] = listen[f]
        if reset and f == reset[1]:
            t.stream_reset(reset[0])
            dec.decode_reset(reset[0])                               # the caller's own decoder follows the stream's life cycle
        carried[f] = state["listen"]

    def after(i):
        nonlocal want
        fr = np.zeros((1, ns, dec.out_stride), dtype=np.uint8)
        ln = np.zeros((1, ns), dtype=np.int32)
        for s in range(ns):
            x = t.frame(s)
            fr[0, s, :len(x)] = np.frombuffer(x, dtype=np.uint8)
            ln[0, s] = len(x)
        got = t.monitor.copy()
        if i == 0:
            assert not ln.any() and not got.view(np.uint8).any()     # the first tick: no frame is final, nothing was looked at
            assert t.monitor_pcm() == (-1, None)
            hist.append(got); reports.append(np.full(ns, EMPTY, dtype=np.uint32))
            return
        rep, _, pcm = dec.decode(fr, ln, want_pcm=True)
        want = ML.fold_python(rep["status"], pcm if what == "audio" else None, rates, want)
        _same(got, want, i)
        hist.append(got); reports.append(rep["status"][0].copy()); pcms.append(pcm[0])
        if what == "audio":
            ls = carried[i] if i < T else state["listen"]
            s, p = t.monitor_pcm()
            if ls < 0:
                assert (s, p) == (-1, None), i
            else:
                assert s == ls and p.tobytes() == pcm[0, ls].tobytes(), (i, ls)

    Loop(t, inter, pipelined, before).go(after)
    final = t.monitor.copy()
    t.close(); dec.close()
    return hist, np.stack(reports), pcms, final


@pytest.mark.parametrize("ngroups,pipelined", [(3, False), (1, True)])
def test_tick_monitor_equals_the_fold_of_a_separate_decode(M, ngroups, pipelined):
    """after every wait; after finish each of the T input frames has come out once, none bad, the first of each stream unchecked.  The
    streams fed digital silence decode to all-zero PCM and count k frame durations; a stream with audio reads 0"""
    T = 8
    hist, rep, pcms, final = _against_batch(M, MIX, T, 9300, "audio", ngroups, pipelined, silent=SILENT)
    assert len(hist) == T + 1
    assert list(final["frames"]) == [T] * len(MIX) and not final["bad_frames"].any() and not final["bad_run"].any()
    assert list(final["flags_seen"]) == [UNCHECKED] * len(MIX) and not final["last_status"].any()
    for s in SILENT:
        assert all(not p[s].any() for p in pcms), s                  # expected of the decoder, not assumed
        for k in range(1, T + 1):
            assert hist[k]["out_silence_ms"][s] == k * (1000 * 1152 // MIX[s][0]) and not hist[k]["out_peak"][s].any(), (s, k)
    loud = [s for s in range(len(MIX)) if s not in SILENT]
    assert not final["out_silence_ms"][loud].any() and (final["out_peak"][loud] > 0).any(axis=1).all()
    mono = [s for s, c in enumerate(MIX) if c[1] == "m"]
    assert not final["out_peak"][mono][:, 1].any()


def test_check_only_leaves_peaks_and_silence_at_zero(M):
    hist, rep, _, final = _against_batch(M, MIX, 5, 9350, "check", 2, True, silent=SILENT)
    assert list(final["frames"]) == [5] * len(MIX) and not final["out_peak"].any() and not final["out_silence_ms"].any()
    assert list(final["flags_seen"]) == [UNCHECKED] * len(MIX)


def test_stream_reset_in_mid_run(M):
    """that stream's next tick shows last_status EMPTY with frames unchanged, the frame after it SCFCRC_UNCHECKED and not bad; every other
    stream's records are those of an undisturbed run"""
    T, r, k = 8, 4, 4
    calm, _, _, _ = _against_batch(M, MIX, T, 9400, "audio", 3)
    hist, rep, _, final = _against_batch(M, MIX, T, 9400, "audio", 3, reset=(r, k))
    assert hist[k][r]["last_status"] == EMPTY and hist[k][r]["frames"] == hist[k - 1][r]["frames"] == k - 1 and not hist[k][r]["out_peak"].any()
    assert hist[k + 1][r]["last_status"] == UNCHECKED and hist[k + 1][r]["frames"] == k and hist[k + 1][r]["bad_frames"] == 0
    assert final[r]["frames"] == T - 1 and final[r]["bad_frames"] == 0 and final[r]["flags_seen"] == UNCHECKED | EMPTY
    others = [s for s in range(len(MIX)) if s != r]
    for i in range(T + 1):
        assert hist[i][others].tobytes() == calm[i][others].tobytes(), i


@pytest.mark.parametrize("stream,byte,tick", [(1, 4, 3), (7, 5, 5)])
def test_one_damaged_byte(M, FI, stream, byte, tick):
    """fault-injection build: one byte of one stream's frame damaged on the device between encode and egress.  The caller receives the
    damaged frame; the record equals the fold of what Batch.decode says of the frames received, at that tick, the next and to the end"""
    T = 8
    hist, rep, _, final = _against_batch(M, MIX, T, 9500, "audio", 3, lib=FI, damage=(stream, byte, 0x40, tick))
    assert rep[tick][stream] & M.DEC_BAD_MASK and hist[tick][stream]["last_status"] == rep[tick][stream]
    assert hist[tick][stream]["bad_frames"] == 1 and hist[tick][stream]["bad_run"] == 1 and not hist[tick][stream]["out_peak"].any()
    assert final[stream]["bad_frames"] == 1 and final[stream]["bad_run"] == 0 and final[stream]["frames"] == T
    assert final[stream]["flags_seen"] == UNCHECKED | rep[tick][stream] | rep[tick + 1][stream]
    others = [s for s in range(len(MIX)) if s != stream]
    assert not final["bad_frames"][others].any() and list(final["flags_seen"][others]) == [UNCHECKED] * len(others)


def test_listen(M):
    """the listened PCM equals Batch.decode's of that stream's frame (checked inside _against_batch at every wait): streams switched
    between ticks and across groups, -1 in between, in both loops; under CHECK the call is refused"""
    T = 9
    plan = {1: 0, 2: 10, 4: -1, 5: 5, 6: 4, 8: 3}
    for pipelined in (False, True):
        _against_batch(M, MIX, T, 9600, "audio", 3, pipelined, listen=plan)
    t = M.Tick(_cfgs(M, MIX[:3]), egress="frames")
    t.enable_monitor("check")
    for s in (0, -1):
        with pytest.raises(M.ToolameError) as e:
            t.monitor_listen(s)
        assert e.value.code == 18
    assert t.monitor_pcm() == (-1, None)
    t.close()
    t = M.Tick(_cfgs(M, MIX[:3]), egress="frames")
    t.enable_monitor("audio")
    for s in (3, -2):
        with pytest.raises(M.ToolameError) as e:
            t.monitor_listen(s)
        assert e.value.code == 18
    t.monitor_listen(2); t.monitor_listen(-1)
    t.close()


def test_enable_rules(M):
    cfgs = _cfgs(M, MIX[:4])
    inter = _inter(MIX[:4], 2, 9700)
    t = M.Tick(cfgs, egress="frames", ngroups=2)
    assert t.monitor is None and t.monitor_pcm() == (-1, None)
    with pytest.raises(M.ToolameError) as e:
        t.monitor_listen(0)                                          # not enabled
    assert e.value.code == 18
    for bad in (0, 3, -1, 4):
        assert t.L.tlb_tick_enable_monitor(t.h, bad) == 18
    t.enable_monitor("audio")
    t.enable_monitor("audio")                                        # (again: no error, no change)
    assert t.L.tlb_tick_enable_monitor(t.h, 1) == 18                 # ... but not another mode
    assert t.monitor.shape == (4,) and not t.monitor.view(np.uint8).any()
    t.pcm[:] = inter[0]
    t.run()
    with pytest.raises(M.ToolameError) as e:
        t.enable_monitor("audio")
    assert e.value.code == 18
    t.close()
    u = M.Tick(cfgs, egress="frames")                                # never enabled: NULL from the accessors, enabling after the first submit refused
    u.pcm[:] = inter[0]
    u.run()
    with pytest.raises(M.ToolameError) as e:
        u.enable_monitor("check")
    assert e.value.code == 18
    u.pcm[:] = inter[1]
    u.run()
    assert u.monitor is None and u.monitor_pcm() == (-1, None) and len(u.frame(0)) > 0
    u.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_node_monitor(M, FI):
    """three shards on the one GPU: records by node-wide index equal ONE Tick's over the same streams, listen follows a stream into its
    shard; a broken shard's streams answer NULL while the others carry on; a restarted shard's records start from zero with the monitor
    on again; a BATCH node refuses"""
    streams = MIX[:9]
    cfgs, ns, T = _cfgs(M, streams), 9, 8
    inter = _inter(streams, T, 9800)
    one = M.Tick(cfgs, egress="frames", ngroups=1)
    one.enable_monitor("audio")
    want, want_pcm = [], []
    for f in range(T):
        one.monitor_listen(f % ns)
        one.pcm[:] = inter[f]
        one.run()
        want.append(one.monitor.copy())
        s, p = one.monitor_pcm()
        want_pcm.append((s, None if p is None else p.copy()))
    one.close()
    nd = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames", ngroups=2, lib=FI)
    assert nd.monitor(0) is None and nd.monitor_pcm() == (-1, None)
    for bad in (0, 3):
        assert nd.L.tlb_node_enable_monitor(nd.h, bad) == 18
    with pytest.raises(M.ToolameError) as e:
        nd.monitor_listen(0)                                         # not enabled
    assert e.value.code == 18
    nd.enable_monitor("audio")
    nd.enable_monitor("audio")
    (f1, n1) = nd.blocks[1]
    in1 = lambda s: f1 <= s < f1 + n1
    for f in range(4):                                               # healthy: equal to the single tick object, listen walks over the shards
        nd.monitor_listen(f % ns)
        nd.set_pcm(inter[f])
        nd.run()
        for s in range(ns):
            assert nd.monitor(s).tobytes() == want[f][s].tobytes(), (f, s)
        s, p = nd.monitor_pcm()
        assert s == want_pcm[f][0] and (p is None) == (want_pcm[f][1] is None) and (p is None or p.tobytes() == want_pcm[f][1].tobytes()), f
    nd.monitor_listen(f1)                                            # a stream of the shard about to break
    nd.fail_next(1, 1)
    nd.set_pcm(inter[4])
    with pytest.raises(M.ToolameError) as e:
        nd.run()
    assert e.value.code == 17 and not nd.shard_ok(1)
    for s in range(ns):
        if in1(s):
            assert nd.monitor(s) is None
        else:
            assert nd.monitor(s).tobytes() == want[4][s].tobytes(), s
    assert nd.monitor_pcm() == (-1, None)
    with pytest.raises(M.ToolameError) as e:
        nd.monitor_listen(f1)
    assert e.value.code == 17
    nd.monitor_listen(0)
    nd.set_pcm(inter[5])
    nd.run()
    s, p = nd.monitor_pcm()
    assert s == 0 and p is not None and nd.monitor(f1) is None and nd.monitor(0).tobytes() == want[5][0].tobytes()
    nd.shard_restart(1)
    for s in range(f1, f1 + n1):
        assert nd.monitor(s).tobytes() == bytes(32)                  # from zero: its streams are fresh
    nd.monitor_listen(f1 + 1)
    for f in (6, 7):
        nd.set_pcm(inter[f])
        nd.run()
    for s in range(ns):
        r = nd.monitor(s)
        if in1(s):
            assert r["frames"] == 1 and r["bad_frames"] == 0 and r["flags_seen"] == UNCHECKED, s       # enabled again: its second tick's frame was looked at
        else:
            assert r.tobytes() == want[7][s].tobytes(), s
    s, p = nd.monitor_pcm()
    assert s == f1 + 1 and p is not None and (np.abs(p.astype(np.int32)).max() > 0)
    nd.close()
    b = M.Node(cfgs, devices=(0, 0), plane="batch")
    assert b.L.tlb_node_enable_monitor(b.h, 2) == 18 and b.L.tlb_node_monitor_listen(b.h, 0) == 18 and b.monitor(0) is None
    b.close()
