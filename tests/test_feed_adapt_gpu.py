"""Adapted feeds on the device (tlb_feed_set_adapted): bit for bit against the lane-loop emulation of the same kernel source on the mixed
stream set of feedadaptlib, against the existing device chain (strict feed decode, numpy channel map, Batch.resample), the transcode chain
against a plain batch given that PCM, the batch-level rules, and the tick and node planes."""
import numpy as np
import pytest

import declib as D
import feedadaptlib as A
import feedlib as F
import resamplelib as R

pytestmark = pytest.mark.gpu
N = A.N
NS = len(A.STREAMS)
ADAPTED = [s for s, st in enumerate(A.STREAMS) if st["adapt"]]
TICK_POISON = 0x5A5A


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def fc_of(M, st):
    return M.FeedConfig(**A.fcfg_of(st))


@pytest.fixture(scope="module")
def run(M):
    """the device run the tests share: the stream set, cut 1 + 5 + 8, into a buffer of random values; the emulation's on the same"""
    sh = A.shared()
    b = M.Batch(A.stream_configs())
    A.set_feeds(b)
    assert b.feed_stride == sh["stride"]
    assert [b.feed_adapted(s) for s in range(NS)] == [st["adapt"] for st in A.STREAMS]
    init = np.random.default_rng(3).integers(-32768, 32768, (A.NTICKS, NS, 2 * N)).astype(np.int16)
    parts, wants, f0 = [], [], 0
    for n in (1, 5, 8):
        wants.append([[b.feed_want(s, a) if st["feed"] else None for a in range(n)] for s, st in enumerate(A.STREAMS)])
        parts.append(b.feed(sh["fr"][f0:f0 + n], sh["ln"][f0:f0 + n], init[f0:f0 + n]))
        f0 += n
    b.close()
    got = tuple(np.concatenate([p[k] for p in parts]) for k in range(2))
    e = A.FeedAdaptEmu(A.STREAMS)
    outs, f0 = [], 0
    for n in (1, 5, 8):
        outs.append(e.decode(sh["fr"][f0:f0 + n], sh["ln"][f0:f0 + n], init[f0:f0 + n]))
        f0 += n
    e.close()
    want = tuple(np.concatenate([p[k] for p in outs]) for k in range(2))
    return dict(init=init, got=got, want=want, wants=wants)


def test_device_equals_emulation_on_the_mixed_batch(run):
    """Test 4.  PCM and reports are the emulation's, bit for bit; what the call must not write is what the buffer held"""
    pcm, rep = run["got"]
    assert pcm.tobytes() == run["want"][0].tobytes()
    assert rep.tobytes() == run["want"][1].tobytes()
    w = A.written(A.STREAMS, A.NTICKS)
    assert np.array_equal(pcm[~w], run["init"][~w])
    for s, st in enumerate(A.STREAMS):
        if not st["feed"]:
            assert (rep["status"][:, s] == D.EMPTY).all()
            continue
        L, Mm = A.lm_of(st)
        assert [int(x) for x in rep["status"][:, s]] == [0 if A.want(f, L, Mm) else D.EMPTY for f in range(A.NTICKS)], s
        assert np.abs(pcm[:, s, :N].astype(int)).max() > 1000, s
        flat = [x for part in run["wants"] for x in part[s]]     # feed_want(s, ahead) before each call
        assert flat == [A.want(f, L, Mm) for f in range(A.NTICKS)] == [M_want(st, f) for f in range(A.NTICKS)], s
    assert np.array_equal(pcm[w], A.shared()["want"][w])          # ... and the numpy oracle's


def M_want(st, f):
    import odr_audioenc_amd as mod
    return mod.feed_want_at(st["feed"][0], st["enc"][0], f)


@pytest.fixture(scope="module")
def chain(M):
    """Test 5's reference, on the device: a strict-feed Batch at each feed's OWN configuration decodes the wanted frames, numpy applies the
    channel map, a Batch with set_source resamples -> int16 [NTICKS][NS][2304] (zeros where nothing is defined; the strict stream decoded likewise)"""
    sh = A.shared()
    fed = [s for s, st in enumerate(A.STREAMS) if st["feed"]]
    d = M.Batch([M.StreamConfig(samplerate=A.STREAMS[s]["feed"][0], mode=A.STREAMS[s]["feed"][1], bitrate=A.STREAMS[s]["feed"][2], psy_model=1) for s in fed])
    for k, s in enumerate(fed):
        d.set_feed(k, fc_of(M, A.STREAMS[s]))
    fr, ln = F.slots_to_arrays([[(b, len(b)) for b in sh["used"][s]] + [(b"", 0)] * (A.NTICKS - len(sh["used"][s])) for s in fed], d.feed_stride)
    inter, rep = d.feed(fr, ln)
    d.close()
    out = np.zeros((A.NTICKS, NS, 2 * N), dtype=np.int16)
    sigs, cfgs, where = [], [], []
    for k, s in enumerate(fed):
        st = A.STREAMS[s]
        fch, sch = A.fcfg_of(st)["channels"], A.enc_nch(st)
        x = inter[:len(sh["used"][s]), k, :N * fch].reshape(-1, fch)
        assert not rep["status"][:len(sh["used"][s]), k].any()
        xm = A.channel_map(x, fch, sch).astype(np.int16)
        if st["feed"][0] == st["enc"][0]:
            y = np.repeat(xm, 2, axis=1) if (fch, sch) == (1, 2) else xm
            out[:, s, :N * sch] = y[:N * A.NTICKS].reshape(A.NTICKS, N * sch)
        else:
            sigs.append(xm); where.append(s)
            cfgs.append(dict(samplerate=st["enc"][0], mode="m" if xm.shape[1] == 1 else "s", source=st["feed"][0]))
    r = M.Batch(R.stream_configs(cfgs))
    for k, c in enumerate(cfgs):
        r.set_source(c["source"], k)
    y = r.resample(R.cut(sigs, cfgs, 0, A.NTICKS))
    r.close()
    for k, s in enumerate(where):
        st = A.STREAMS[s]
        if xm_is_dup(st):
            out[:, s] = np.repeat(y[:, k, :N], 2, axis=1)
        else:
            out[:, s, :N * A.enc_nch(st)] = y[:, k, :N * A.enc_nch(st)]
    return out


def xm_is_dup(st):
    return A.fcfg_of(st)["channels"] == 1 and A.enc_nch(st) == 2


def test_device_equals_the_existing_device_chain(run, chain):
    """Test 5."""
    w = A.written(A.STREAMS, A.NTICKS)
    for s, st in enumerate(A.STREAMS):
        if st["feed"]:
            assert np.array_equal(run["got"][0][:, s][w[:, s]], chain[:, s][w[:, s]]), s


def test_transcode_equals_a_plain_batch_given_the_chains_pcm(M, chain):
    """Test 6.  adapted feed -> ingest -> encode: byte-identical frames"""
    sh = A.shared()
    plain = M.Batch(A.stream_configs())
    pcm, _ = plain.ingest(chain)
    want, _ = plain.encode(pcm)
    want_last = plain.flush()
    plain.close()
    b = M.Batch(A.stream_configs())
    A.set_feeds(b)
    inter, _ = b.feed(sh["fr"], sh["ln"])
    planar, _ = b.ingest(inter)
    assert np.array_equal(planar, pcm)
    got, _ = b.encode(planar)
    got_last = b.flush()
    b.close()
    assert got == want and got_last == want_last and all(len(x) > 0 for x in got)


def test_rules(M, run):
    """Test 7."""
    sh = A.shared()
    b = M.Batch(A.stream_configs())
    st0, st1 = A.STREAMS[0], A.STREAMS[1]
    for s, cfg, code in ((0, fc_of(M, st0), 1), (1, M.FeedConfig(48000, 128, 2), 2)):       # without adapt: the strict refusals
        with pytest.raises(M.ToolameError) as e:
            b.set_feed(s, cfg)
        assert e.value.code == code
    for s, cfg, code in ((2, fc_of(M, st0), 1), (0, M.FeedConfig(48000, 100, 2), 4), (0, M.FeedConfig(44100, 128, 3), 2), (0, M.FeedConfig(8000, 64, 2), 1),
                         (-1, fc_of(M, st0), 1), (NS, fc_of(M, st0), 18)):
        with pytest.raises(M.ToolameError) as e:
            b.set_feed(s, cfg, adapt=True)
        assert e.value.code == code, (s, cfg)
    assert b.feed_stride == 0 and all(b.get_feed(s) is None and not b.feed_adapted(s) for s in range(NS))      # nothing changed
    with pytest.raises(M.ToolameError) as e:
        b.feed_want(0)                                           # no feed
    assert e.value.code == 18
    # a matching configuration through adapt=True IS the strict feed: the strict path's bytes
    b.set_feed(6, fc_of(M, A.STREAMS[6]), adapt=True)
    assert not b.feed_adapted(6) and b.feed_want(6) == 1 and b.feed_want(6, 5) == 1
    fr, ln = F.slots_to_arrays([sh["lists"][6]], b.feed_stride)
    frames = np.zeros((A.NTICKS, NS, b.feed_stride), dtype=np.uint8); lens = np.zeros((A.NTICKS, NS), dtype=np.int32)
    frames[:, 6], lens[:, 6] = fr[:, 0], ln[:, 0]
    pcm, rep = b.feed(frames, lens)
    assert np.array_equal(pcm[:, 6], run["got"][0][:, 6]) and not rep["status"][:, 6].any()
    # reconfigure: an adapted feed stays while (Fs, new Es) is a legal pair, whatever the channels, with fresh state; else it goes
    b.set_feed(0, fc_of(M, st0), adapt=True)                     # 44.1 kHz two channels on 48 kHz 's'
    one = b.feed(_only(sh, 0, b, 3), _only_len(sh, 0, 3))
    assert b.feed_want(0) == 1 and b.feed_adapted(0)
    b.stream_reconfigure(0, M.StreamConfig(samplerate=48000, mode="m", bitrate=64, psy_model=1))
    assert b.feed_adapted(0) and b.get_feed(0) is not None
    again = b.feed(_only(sh, 0, b, 3), _only_len(sh, 0, 3))     # tick 0 again, now mapped to one channel
    want = A.oracle_pcm(sh["used"][0][:4], dict(A.STREAMS[0], enc=(48000, "m")), 3)
    assert np.array_equal(again[0][:, 0, :N], want[:3, :N]) and not np.array_equal(again[0][:, 0, :N], one[0][:, 0, :N])
    b.stream_reconfigure(0, M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1))       # 44.1 -> 24 kHz: no pair
    assert not b.feed_adapted(0) and b.get_feed(0) is None
    b.set_feed(3, fc_of(M, A.STREAMS[3]), adapt=True)            # 16 kHz on 24 kHz
    for a in range(8):
        assert b.feed_want(3, a) == M.feed_want_at(16000, 24000, a)
    b.feed(_only(sh, 3, b, 2), _only_len(sh, 3, 2))
    assert [b.feed_want(3, a) for a in range(4)] == [M.feed_want_at(16000, 24000, 2 + a) for a in range(4)] == [0, 1, 1, 0]
    b.feed_reset(3)
    assert b.feed_want(3) == 1 and b.feed_want(3, 2) == 0
    b.set_feed(3, None, adapt=True)
    assert b.get_feed(3) is None and not b.feed_adapted(3)
    b.close()


def _only(sh, s, b, n):
    fr = np.zeros((n, NS, b.feed_stride), dtype=np.uint8)
    w = min(b.feed_stride, sh["fr"].shape[2])
    fr[:, s, :w] = sh["fr"][:n, s, :w]
    return fr


def _only_len(sh, s, n):
    ln = np.zeros((n, NS), dtype=np.int32)
    ln[:, s] = sh["ln"][:n, s]
    return ln


# ---- the tick plane: two groups of four, group 0 all fed (adapted), group 1 mixed (adapted, adapted, strict, none) ----------------------------
def tick_fill(t, f, live):
    """tick f's input as the caller of an adapted feed makes it: a frame where one is wanted, nothing elsewhere"""
    sh = A.shared()
    t.pcm[:] = TICK_POISON
    t.pcm[NS - 1] = live[f]
    fr, ln = t.feed, t.feed_len
    assert fr is not None and not ln.any()
    for s, st in enumerate(A.STREAMS):
        if not st["feed"]:
            continue
        L, Mm = A.lm_of(st)
        assert t.feed_want(s) == A.want(f, L, Mm), (f, s)
        b, n = sh["lists"][s][f]
        if t.feed_want(s):
            fr[s, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            ln[s] = n


def live_pcm():
    from pcmgen import gen_pcm
    return F.interleave(gen_pcm(977, 0, 0, A.NTICKS), 2)


def test_tick_with_adapted_feeds_equals_tick_given_the_batch_levels_pcm(M, run):
    """Test 8.  Fourteen ticks overlapped; frames and peaks equal a tick object given the PCM of the batch-level run; feed_want per tick;
    the reports are the batch level's"""
    live = live_pcm()
    want_pcm = run["got"][0].copy()
    want_pcm[:, NS - 1] = live
    kw = dict(egress="frames", ngroups=2)
    a, b = M.Tick(A.stream_configs(), **kw), M.Tick(A.stream_configs(), **kw)
    A.set_feeds(a)
    for x in (a.enable_short_reads, lambda: a.set_source(44100, 7)):        # adapted feeds exclude short reads and sources, as feeds do
        with pytest.raises(M.ToolameError) as e:
            x()
        assert e.value.code == 18
    got, exp, reps = [], [], []

    def submit(f):
        tick_fill(a, f, live)
        b.pcm[:] = want_pcm[f]
        a.submit(); b.submit()

    def wait():
        a.wait(); b.wait()
        got.append([(a.frame(s), tuple(int(x) for x in a.peaks[s])) for s in range(NS)])
        exp.append([(b.frame(s), tuple(int(x) for x in b.peaks[s])) for s in range(NS)])
        reps.append(a.feed_report.copy())
    submit(0); submit(1)
    with pytest.raises(M.ToolameError) as e:                     # a tick is in flight
        a.set_feed(0, fc_of(M, A.STREAMS[0]), adapt=True)
    assert e.value.code == 18
    wait()
    for f in range(2, A.NTICKS):
        submit(f); wait()
    wait()
    a.finish(); b.finish()
    got.append([(a.frame(s), ()) for s in range(NS)]); exp.append([(b.frame(s), ()) for s in range(NS)])
    for f in range(A.NTICKS + 1):
        for s in range(NS):
            assert got[f][s] == exp[f][s], (f, s)
        if f >= 1:
            assert all(len(x[0]) > 0 for x in got[f])
    assert np.array_equal(np.stack(reps)["status"], run["got"][1]["status"])
    a.close(); b.close()
    t = M.Tick(A.stream_configs(), **kw)
    t.set_source(44100, 7)
    with pytest.raises(M.ToolameError) as e:                     # ... from the other side
        t.set_feed(0, fc_of(M, A.STREAMS[0]), adapt=True)
    assert e.value.code == 18 and t.feed is None
    t.close()


def test_a_refused_adapted_opt_in_leaves_the_object_healthy(M):
    """the fault-injection build refuses the nth allocation of the memory owner for nth = 1, 2, ... until tlb_tick_set_feed_adapted is
    accepted: every refusal answers TLB_ERR_HIP and leaves no feed and a healthy object, which then produces a twin's bytes"""
    sh = A.shared()
    FI = M.load_fault_library()
    st = A.STREAMS[0]
    scfgs = A.stream_configs([st] * 4)
    fc = fc_of(M, st)
    t, twin = M.Tick(scfgs, egress="frames", ngroups=2, lib=FI), M.Tick(scfgs, egress="frames", ngroups=2, lib=FI)
    twin.set_feed(-1, fc, adapt=True)
    refused = 0
    try:
        for nth in range(1, 97):
            assert FI.tlb_debug_alloc_fail_next(nth) == 0
            try:
                t.set_feed(-1, fc, adapt=True)
                break
            except M.ToolameError as e:
                assert e.code == 17, (nth, e.code)
            assert t.feed is None and t.feed_report is None and t.feed_stride == 0 and t.status() == 0, nth
            refused += 1
        else:
            pytest.fail("not accepted")
    finally:
        FI.tlb_debug_alloc_fail_next(0)
    assert refused >= 8                                          # the strict path's, and the queue state and plane of each group's batch
    for f in range(3):
        for x in (t, twin):
            b = sh["used"][0][f]
            assert [x.feed_want(s) for s in range(4)] == [1] * 4
            x.feed[:, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            x.feed_len[:] = len(b)
            x.run()
        assert not t.feed_report["status"].any()
        for s in range(4):
            assert t.frame(s) == twin.frame(s) and (f == 0 or len(t.frame(s)) > 0), (f, s)
    t.close(); twin.close()


def test_node_routes_adapted_feeds_and_restores_them_on_a_restart(M):
    """Test 9.  devices = (0, 0): two shards of four streams; frames, reports and feed_want equal one tick object's; a restarted shard has
    its adapted feeds again at tick 0; a BATCH-plane node refuses feed_want"""
    sh = A.shared()
    live = live_pcm()
    scfgs = A.stream_configs()
    nd = M.Node(scfgs, devices=(0, 0), plane="tick", egress="frames")
    t = M.Tick(scfgs, egress="frames", ngroups=2)
    assert M.node_partition(NS, 2) == [(0, 4), (4, 4)]
    with pytest.raises(M.ToolameError) as e:
        nd.set_feed(0, fc_of(M, A.STREAMS[0]))                   # the strict entry point still refuses
    assert e.value.code == 1
    with pytest.raises(M.ToolameError) as e:
        nd.set_feed(2, fc_of(M, A.STREAMS[0]), adapt=True)       # 44.1 kHz for 24 kHz
    assert e.value.code == 1
    A.set_feeds(nd); A.set_feeds(t)

    def node_fill(f, tick_of):
        row = np.full((NS, 2 * N), TICK_POISON, dtype=np.int16)
        row[NS - 1] = live[f]
        nd.set_pcm(row)
        for s, st in enumerate(A.STREAMS):
            if not st["feed"]:
                continue
            L, Mm = A.lm_of(st)
            assert nd.feed_want(s) == A.want(tick_of(s), L, Mm), (f, s)
            if nd.feed_want(s):
                b, n = sh["lists"][s][tick_of(s)]
                slot, ln = nd.feed(s), nd.feed_len(s)
                slot[:len(b)] = np.frombuffer(b, dtype=np.uint8)
                ln[0] = n
    for f in range(4):
        node_fill(f, lambda s: f)
        tick_fill(t, f, live)
        nd.run(); t.run()
        for s in range(NS):
            assert nd.frame(s) == t.frame(s), (f, s)
            assert nd.feed_report(s) == t.feed_report[s], (f, s)
    nd.shard_restart(0)                                          # block 0 starts again: its adapted feeds at tick 0, block 1 goes on at tick 4
    fresh = M.Tick(scfgs[:4], egress="frames")
    A.set_feeds(fresh, A.STREAMS[:4])
    for k in range(3):
        node_fill(4 + k, lambda s: k if s < 4 else 4 + k)
        tick_fill(t, 4 + k, live)
        fresh.pcm[:] = TICK_POISON
        for s in range(4):
            b, n = sh["lists"][s][k]
            assert fresh.feed_want(s) == nd_want(s, k)
            if fresh.feed_want(s):
                fresh.feed[s, :len(b)] = np.frombuffer(b, dtype=np.uint8)
                fresh.feed_len[s] = n
        nd.run(); t.run(); fresh.run()
        for s in range(NS):
            x = fresh if s < 4 else t
            assert nd.frame(s) == x.frame(s), (k, s)
            assert nd.feed_report(s) == x.feed_report[s], (k, s)
    nd.close(); t.close(); fresh.close()
    nb = M.Node(scfgs, devices=(0, 0), plane="batch")
    nb.set_feed(0, fc_of(M, A.STREAMS[0]), adapt=True)           # tlb_feed_set_adapted of the shard's batch
    with pytest.raises(M.ToolameError) as e:
        nb.feed_want(0)
    assert e.value.code == 18
    nb.close()


def nd_want(s, f):
    return A.want(f, *A.lm_of(A.STREAMS[s]))
