"""Down feeds on the device (tlb_feed_down_*): bit for bit against the lane-loop emulation of the same kernel source on the stream set of
feeddownlib under its three cuts, against the existing device chain (strict feed decode at the feed's rate, numpy channel map,
Batch.decimate), the transcode chain against a plain 24 kHz batch given the oracle's PCM, a batch that holds every source family, the wrap
of the position, and the batch-level rules."""
import numpy as np
import pytest

import decimatelib as DC
import declib as D
import feedadaptlib as FA
import feeddownlib as A
import feedlib as F

pytestmark = pytest.mark.gpu
N = A.N
NS = len(A.STREAMS)
FED = [s for s, st in enumerate(A.STREAMS) if st["feed"]]


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def device_cuts(M, cuts, init):
    """the stream set on a Batch, its ticks cut into calls -> (pcm, report, down_feed_want(s, ahead) before each call)"""
    sh = A.shared()
    b = M.Batch(A.stream_configs())
    A.set_down_feeds(b)
    assert b.down_feed_stride == sh["stride"] and b.feed_stride == 0
    parts, wants, f0 = [], [], 0
    for n in cuts:
        wants.append([[b.down_feed_want(s, a) if st["feed"] else None for a in range(n)] for s, st in enumerate(A.STREAMS)])
        parts.append(b.down_feed(sh["fr"][f0:f0 + n], sh["ln"][f0:f0 + n], init[f0:f0 + n]))
        f0 += n
    b.close()
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), wants


@pytest.fixture(scope="module")
def run(M):
    """what the tests share: the buffer of random values the calls write into, the emulation's result on it, the device's under cut 1 + 3 + 4"""
    sh = A.shared()
    init = np.random.default_rng(3).integers(-32768, 32768, (A.NTICKS, NS, 2 * N)).astype(np.int16)
    e = A.FeedDownEmu(A.STREAMS)
    want = e.decode(sh["fr"], sh["ln"], init)
    e.close()
    pcm, rep, wants = device_cuts(M, (1, 3, 4), init)
    return dict(init=init, want=want, got=(pcm, rep), wants=wants)


@pytest.mark.parametrize("cuts", A.CUTS, ids=["8", "1+3+4", "8x1"])
def test_device_equals_emulation(M, run, cuts):
    """PCM and reports are the emulation's, bit for bit, under every cut; what the call must not write is what the buffer held"""
    pcm, rep, wants = (run["got"] + (run["wants"],)) if cuts == (1, 3, 4) else device_cuts(M, cuts, run["init"])
    assert pcm.tobytes() == run["want"][0].tobytes()
    assert rep.tobytes() == run["want"][1].tobytes()
    w = A.written(A.STREAMS, A.NTICKS)
    assert np.array_equal(pcm[~w], run["init"][~w])
    assert np.array_equal(pcm[w], A.shared()["want"][w])          # ... and the numpy oracle's
    wanted, other = A.expected_status(A.STREAMS, A.shared()["ln"])
    assert (rep["status"][wanted] == 0).all() and np.array_equal(rep["status"][~wanted], other[~wanted])
    for s in FED:
        st = A.STREAMS[s]
        L, Mm = A.lm_of(st)
        assert np.abs(pcm[:, s, :N].astype(int)).max() > 1000, s
        flat = [x for part in wants for x in part[s]]             # down_feed_want(s, ahead) before each call
        assert flat == [A.want(f, L, Mm) for f in range(A.NTICKS)] == [M.down_feed_want_at(st["feed"][0], A.ES, f) for f in range(A.NTICKS)], s


@pytest.fixture(scope="module")
def chain(M):
    """the reference on the device: a strict-feed Batch at each feed's OWN configuration decodes the wanted frames, numpy applies the channel
    map, a Batch with set_down_source decimates -> int16 [NTICKS][NS][2304] (zeros where nothing is defined)"""
    sh = A.shared()
    nmax = max(len(sh["used"][s]) for s in FED)
    d = M.Batch([M.StreamConfig(samplerate=A.STREAMS[s]["feed"][0], mode=A.STREAMS[s]["feed"][1], bitrate=A.STREAMS[s]["feed"][2], psy_model=1) for s in FED])
    for k, s in enumerate(FED):
        d.set_feed(k, A.feed_config(A.STREAMS[s]))
    fr, ln = F.slots_to_arrays([[(b, len(b)) for b in sh["used"][s]] + [(b"", 0)] * (nmax - len(sh["used"][s])) for s in FED], d.feed_stride)
    inter, rep = d.feed(fr, ln)
    d.close()
    sigs, cfgs = [], []
    for k, s in enumerate(FED):
        st = A.STREAMS[s]
        fch, sch = A.fcfg_of(st)["channels"], A.enc_nch(st)
        assert not rep["status"][:len(sh["used"][s]), k].any()
        xm = A.channel_map(inter[:len(sh["used"][s]), k, :N * fch].reshape(-1, fch), fch, sch).astype(np.int16)
        sigs.append(xm)
        cfgs.append(dict(samplerate=A.ES, mode="m" if xm.shape[1] == 1 else "s", source=st["feed"][0]))
    r = M.Batch(DC.stream_configs(cfgs))
    for k, c in enumerate(cfgs):
        r.set_down_source(c["source"], k)
    y = r.decimate(DC.cut(sigs, cfgs, 0, A.NTICKS))
    r.close()
    out = np.zeros((A.NTICKS, NS, 2 * N), dtype=np.int16)
    for k, s in enumerate(FED):
        st = A.STREAMS[s]
        if A.fcfg_of(st)["channels"] == 1 and A.enc_nch(st) == 2:
            out[:, s] = np.repeat(y[:, k, :N], 2, axis=1)
        else:
            out[:, s, :N * A.enc_nch(st)] = y[:, k, :N * A.enc_nch(st)]
    return out


def test_device_equals_the_existing_device_chain(run, chain):
    w = A.written(A.STREAMS, A.NTICKS)
    for s in FED:
        assert np.array_equal(run["got"][0][:, s][w[:, s]], chain[:, s][w[:, s]]), s


def test_transcode_equals_a_plain_batch_given_the_oracles_pcm(M):
    """down feed -> ingest -> encode: the frames of a plain 24 kHz batch given the numpy oracle's PCM, byte for byte"""
    sh = A.shared()
    plain = M.Batch(A.stream_configs())
    pcm, _ = plain.ingest(sh["want"])
    want, _ = plain.encode(pcm)
    want_last = plain.flush()
    plain.close()
    b = M.Batch(A.stream_configs())
    A.set_down_feeds(b)
    inter, _ = b.down_feed(sh["fr"], sh["ln"])
    planar, _ = b.ingest(inter)
    assert np.array_equal(planar, pcm)
    got, _ = b.encode(planar)
    got_last = b.flush()
    b.close()
    assert got == want and got_last == want_last and all(len(x) > 0 for x in got)


def test_every_source_family_in_one_batch(M, run):
    """streams 0 .. 6 as in the set, then a strict 24 kHz feed, an adapted 22.05 -> 24 kHz feed and a set_down_source(48000) stream: each
    family's output is what it is in a batch of its own"""
    sh, fa = A.shared(), FA.shared()
    strict = (24000, "m", 32, 0)
    st_ad = FA.STREAMS[2]                                         # 22.05 kHz 'm' 32 -> 24 kHz 's'
    assert st_ad["feed"][0] == 22050 and st_ad["enc"] == (24000, "s")
    strict_fr = F.oracle_frames(strict, F.case_pcm(91, strict, A.NTICKS))
    sfc, afc = M.FeedConfig(**F.feed_cfg_of(strict)), M.FeedConfig(**FA.fcfg_of(st_ad))
    sig = DC.signal(dict(mode="s"), "noise", DC.total_need(dict(source=48000, samplerate=24000), A.NTICKS), seed=4)
    extra = [M.StreamConfig(samplerate=24000, mode="m", bitrate=32, psy_model=1), M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1),
             M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1)]

    def feeds_of(b, s_strict, s_ad):
        """the strict and the adapted stream's eight ticks through b.feed -> pcm [8][nstreams][2304]"""
        b.set_feed(s_strict, sfc)
        b.set_feed(s_ad, afc, adapt=True)
        fr = np.zeros((A.NTICKS, b.nstreams, b.feed_stride), dtype=np.uint8); ln = np.zeros((A.NTICKS, b.nstreams), dtype=np.int32)
        k = 0
        for f in range(A.NTICKS):
            fr[f, s_strict, :len(strict_fr[f])] = np.frombuffer(strict_fr[f], dtype=np.uint8); ln[f, s_strict] = len(strict_fr[f])
            if b.feed_want(s_ad, f):
                x = fa["used"][2][k]; k += 1
                fr[f, s_ad, :len(x)] = np.frombuffer(x, dtype=np.uint8); ln[f, s_ad] = len(x)
        return fr, ln

    def wide_of(b, s):
        w = np.zeros((A.NTICKS, b.nstreams, DC.WIDE), dtype=np.int16)
        w[:, s, :] = DC.cut([sig], [dict(source=48000, samplerate=24000, mode="s")], 0, A.NTICKS)[:, 0]
        return w
    alone = M.Batch(extra)
    alone.set_down_source(48000, 2)
    fr, ln = feeds_of(alone, 0, 1)
    want_feed, want_rep = alone.feed(fr, ln)
    want_dec = alone.decimate(wide_of(alone, 2))
    alone.close()
    b = M.Batch(A.stream_configs() + extra)
    A.set_down_feeds(b)
    b.set_down_source(48000, NS + 2)
    fr, ln = feeds_of(b, NS, NS + 1)
    dfr = np.zeros((A.NTICKS, NS + 3, 2, b.down_feed_stride), dtype=np.uint8); dln = np.zeros((A.NTICKS, NS + 3, 2), dtype=np.int32)
    dfr[:, :NS], dln[:, :NS] = sh["fr"], sh["ln"]
    init = np.zeros((A.NTICKS, NS + 3, 2 * N), dtype=np.int16)
    init[:, :NS] = run["init"]
    pcm, rep = b.down_feed(dfr, dln, init)                        # the three families in the order a caller may choose: each leaves the others' slots alone
    pcm, frep = b.feed(fr, ln, pcm)
    pcm = b.decimate(wide_of(b, NS + 2), pcm)
    b.close()
    assert np.array_equal(pcm[:, :NS], run["want"][0]) and rep[:, :NS].tobytes() == run["want"][1].tobytes()
    assert (rep["status"][:, NS:] == D.EMPTY).all()
    assert np.array_equal(pcm[:, NS, :N], want_feed[:, 0, :N]) and np.array_equal(pcm[:, NS + 1], want_feed[:, 1]) and np.array_equal(pcm[:, NS + 2], want_dec[:, 2])
    assert np.array_equal(frep["status"][:, NS:NS + 2], want_rep["status"][:, :2]) and np.abs(want_feed[:, 1].astype(int)).max() > 1000


def test_the_position_wraps_at_80(M):
    """one 44.1 kHz stream over 82 ticks cut (79, 3): the emulation's output, across the wrap of the position between the calls"""
    st = A.STREAMS[2]
    nt = 82
    L, Mm = A.lm_of(st)
    sl = A.slots_of(A.feed_frames(2, st, A.K(nt - 1, L, Mm)), L, Mm, nt)
    e = A.FeedDownEmu([st])
    fr, ln = A.slots_to_arrays([sl], e.stride)
    want_pcm, want_rep = e.run_cuts(fr, ln, (79, 3))
    assert e.pos(0) == 2
    e.close()
    b = M.Batch(A.stream_configs([st]))
    b.set_down_feed(0, A.feed_config(st))
    a = b.down_feed(fr[:79], ln[:79])
    assert [b.down_feed_want(0, x) for x in range(3)] == [A.want(79 + x, L, Mm) for x in range(3)]
    c = b.down_feed(fr[79:], ln[79:])
    assert [b.down_feed_want(0, x) for x in range(8)] == [A.want(2 + x, L, Mm) for x in range(8)]
    b.close()
    pcm, rep = np.concatenate([a[0], c[0]]), np.concatenate([a[1], c[1]])
    assert np.array_equal(pcm[:, 0, :2 * N], want_pcm[:, 0, :2 * N]) and rep.tobytes() == want_rep.tobytes()
    assert not rep["status"][:, 0, 0].any() and np.abs(pcm[79:].astype(int)).max() > 1000


def test_rules(M, run):
    """what a down feed must fit; one source per stream, from both sides, with nothing changed; the life-cycle calls; reconfiguration"""
    sh = A.shared()
    b = M.Batch(A.stream_configs() + [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1)])
    fc0 = A.feed_config(A.STREAMS[0])
    for s, cfg, code in ((NS, fc0, 1), (0, M.FeedConfig(24000, 64, 2), 1), (0, M.FeedConfig(22050, 64, 2), 1), (0, M.FeedConfig(48000, 100, 2), 4),
                         (0, M.FeedConfig(48000, 128, 3), 2), (-1, fc0, 1), (NS + 1, fc0, 18)):
        with pytest.raises(M.ToolameError) as e:
            b.set_down_feed(s, cfg)
        assert e.value.code == code, (s, cfg)
    assert b.down_feed_stride == 0 and all(b.down_feed_cfg(s) is None for s in range(NS + 1))      # nothing changed
    b.set_down_feed(0, None)                                      # removing what is not there is no down feed
    with pytest.raises(M.ToolameError) as e:
        b.down_feed_want(0)
    assert e.value.code == 18
    with pytest.raises(M.ToolameError) as e:                      # no stream has a down feed
        b.down_feed(np.zeros((1, NS + 1, 2, 0), dtype=np.uint8), np.zeros((1, NS + 1, 2), dtype=np.int32))
    assert e.value.code == 18
    # one source per stream: a down feed is refused beside each other family ...
    b.set_feed(5, M.FeedConfig(24000, 32, 1)); b.set_feed(4, M.FeedConfig(22050, 32, 1), adapt=True); b.set_source(16000, 3); b.set_down_source(48000, 2)
    for s in (5, 4, 3, 2):
        with pytest.raises(M.ToolameError) as e:
            b.set_down_feed(s, fc0)
        assert e.value.code == 18 and b.down_feed_cfg(s) is None, s
    with pytest.raises(M.ToolameError) as e:
        b.set_down_feed(-1, fc0)                                  # ... and for every stream at once (the 48 kHz stream refuses first: no pair)
    assert e.value.code == 1 and b.down_feed_stride == 0
    assert b.get_feed(5) is not None and b.feed_adapted(4) and b.source(3) == 16000 and b.down_source(2) == 48000
    # ... and each other family beside a down feed
    b.set_down_feed(0, fc0); b.set_down_feed(1, A.feed_config(A.STREAMS[2]))
    assert b.down_feed_stride == 576 and b.down_feed_cfg(1).samplerate == 44100 and b.get_feed(0) is None
    for x in (lambda: b.set_feed(0, M.FeedConfig(24000, 64, 2)), lambda: b.set_feed(0, M.FeedConfig(22050, 64, 2), adapt=True),
              lambda: b.set_source(22050, 0), lambda: b.set_down_source(48000, 0), lambda: b.set_down_source(44100, 1)):
        with pytest.raises(M.ToolameError) as e:
            x()
        assert e.value.code == 18
    assert b.get_feed(0) is None and b.source(0) == 0 and b.down_source(0) == 0 and b.down_source(1) == 0 and b.down_feed_cfg(0) is not None
    b.set_feed(0, None); b.set_source(0, 0); b.set_down_source(0, 0)                 # "off" is not a source
    # the schedule follows the calls and the resets
    fr = np.zeros((4, NS + 1, 2, 576), dtype=np.uint8); ln = np.zeros((4, NS + 1, 2), dtype=np.int32)
    fr[:, 1], ln[:, 1] = sh["fr"][:4, 2], sh["ln"][:4, 2]
    one, _ = b.down_feed(fr, ln)
    mono = A.oracle_pcm(sh["used"][2][:8], dict(A.STREAMS[2], mode="m"), 4)      # (stream 1 of the batch has one channel: the 44.1 kHz feed is mapped)
    assert np.array_equal(one[:, 1], mono)
    assert [b.down_feed_want(1, a) for a in range(4)] == [M.down_feed_want_at(44100, 24000, 4 + a) for a in range(4)] == [2, 2, 1, 2]
    for reset in (lambda: b.down_feed_reset(1), lambda: b.stream_reset(1), lambda: b.reset()):
        reset()
        assert [b.down_feed_want(1, a) for a in range(7)] == [2, 2, 2, 2, 2, 2, 1]
        again, _ = b.down_feed(fr[:2], ln[:2])
        assert np.array_equal(again[:, 1], one[:2, 1])            # tick 0 again, after silence
    # reconfigure: a down feed stays while (Fs, new Es) is a legal pair, whatever the channels, with fresh state; else it goes
    b.down_feed(fr[:2], ln[:2])
    b.stream_reconfigure(1, M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1))
    assert b.down_feed_cfg(1) is not None and b.down_feed_want(1) == 2
    two, _ = b.down_feed(fr[:3], ln[:3])                          # tick 0 again, now with both channels
    assert np.array_equal(two[:, 1], sh["want"][:3, 2]) and not np.array_equal(two[:, 1, :N], mono[:3, :N])
    b.stream_reconfigure(1, M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1))
    assert b.down_feed_cfg(1) is None and b.down_feed_cfg(0) is not None and b.down_feed_stride == 576
    b.set_down_feed(0, None)
    assert b.down_feed_stride == 0
    b.close()


def test_a_batch_without_a_down_feed_is_what_it_was(M):
    """an object that never sets a down feed (or removes one it never had, or sets one and removes it again): feeds, decimator and encoder
    compute what they compute on a batch nothing of this touched.  What it computes is checked; which device calls it queues is the
    launch's own (tlb_feed_down_device is the only entry that queues the down-feed kernels, and it refuses without a down feed)."""
    from pcmgen import gen_pcm
    scfgs = A.stream_configs(A.STREAMS[:3])
    inter = np.stack([F.interleave(gen_pcm(720 + s, 0, 0, 4), A.enc_nch(A.STREAMS[s])) for s in range(3)], axis=1)
    outs = []
    for touch in (False, True):
        b = M.Batch(scfgs)
        if touch:
            b.set_down_feed(-1, None)
            b.set_down_feed(0, A.feed_config(A.STREAMS[0])); b.set_down_feed(0, None)
            assert b.down_feed_stride == 0
            b.set_down_source(48000, 0); b.set_down_source(0, 0)  # ... so the other families are not refused
        pcm, peaks = b.ingest(inter)
        got, _ = b.encode(pcm)
        outs.append((pcm.tobytes(), peaks.tobytes(), got, b.flush()))
        b.close()
    assert outs[0] == outs[1] and all(len(x) > 0 for x in outs[0][2])


# ---- the tick plane: two groups, group 0 all fed (it copies no PCM), group 1 mixed (fed, fed, none) ------------------------------------
TICK_POISON = 0x5A5A


def tick_fill(t, f, live):
    """tick f's input as the caller of a down feed makes it: one or two frames as down_feed_want says, poison where no PCM is read"""
    sh = A.shared()
    t.pcm[:] = TICK_POISON
    t.pcm[NS - 1] = live[f]
    fr, ln = t.down_feed, t.down_feed_len
    assert fr is not None and fr.shape == (NS, 2, t.down_feed_stride) and not ln.any()
    for s in FED:
        L, Mm = A.lm_of(A.STREAMS[s])
        assert t.down_feed_want(s) == A.want(f, L, Mm), (f, s)
        for j in range(t.down_feed_want(s)):
            b, n = sh["lists"][s][f][j]
            fr[s, j, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            ln[s, j] = n


def test_tick_with_down_feeds_equals_tick_given_the_oracles_pcm(M, run):
    """eight ticks overlapped; frames and peaks equal a tick object given the numpy oracle's PCM at 24 kHz; down_feed_want per tick; the
    reports are the batch level's; the exclusions from both sides"""
    from pcmgen import gen_pcm
    sh = A.shared()
    live = F.interleave(gen_pcm(977, 0, 0, A.NTICKS), 2)
    want_pcm = sh["want"].copy()
    want_pcm[:, NS - 1] = live
    kw = dict(egress="frames", ngroups=2)
    a, b = M.Tick(A.stream_configs(), **kw), M.Tick(A.stream_configs(), **kw)
    assert a.down_feed is None and a.down_feed_len is None and a.down_feed_report is None and a.down_feed_stride == 0
    A.set_down_feeds(a)
    assert a.down_feed_stride == sh["stride"]
    fc0 = A.feed_config(A.STREAMS[0])
    for x in (a.enable_short_reads, lambda: a.set_source(22050, 6), lambda: a.set_down_source(48000, 6), lambda: a.set_feed(6, M.FeedConfig(24000, 64, 2)),
              lambda: a.set_feed(6, M.FeedConfig(22050, 64, 2), adapt=True)):      # down feeds exclude short reads, sources, down sources and feeds
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
        reps.append(a.down_feed_report.copy())
    submit(0); submit(1)
    assert a.down_feed is None
    with pytest.raises(M.ToolameError) as e:                     # a tick is in flight
        a.set_down_feed(0, fc0)
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
    for other in (lambda t: t.enable_short_reads(), lambda t: t.set_source(22050, 6), lambda t: t.set_down_source(48000, 6),
                  lambda t: t.set_feed(6, M.FeedConfig(24000, 64, 2))):
        t = M.Tick(A.stream_configs(), **kw)
        other(t)
        with pytest.raises(M.ToolameError) as e:                 # ... from the other side
            t.set_down_feed(0, fc0)
        assert e.value.code == 18 and t.down_feed is None and t.down_feed_stride == 0
        t.close()


def test_tick_reset_and_reconfigure_with_a_down_feed(M):
    """stream_reset puts the stream's schedule back to tick 0; a reconfiguration the feed's rate no longer pairs with removes it"""
    sh = A.shared()
    st = A.STREAMS[4]                                             # 32 kHz: wants 2, 1, 1
    t = M.Tick(A.stream_configs([st, A.STREAMS[6]]), egress="frames")
    t.set_down_feed(0, A.feed_config(st))
    seen = []
    for f in range(2):
        seen.append(t.down_feed_want(0))
        for j in range(seen[-1]):
            b, n = sh["lists"][4][f][j]
            t.down_feed[0, j, :len(b)] = np.frombuffer(b, dtype=np.uint8); t.down_feed_len[0, j] = n
        t.run()
        assert not t.down_feed_report["status"][0, :seen[-1]].any() and (t.down_feed_report["status"][1] == D.EMPTY).all()
    assert seen == [2, 1] and t.down_feed_want(0) == 1
    t.stream_reset(0)
    assert t.down_feed_want(0) == 2
    t.stream_reconfigure(0, M.StreamConfig(samplerate=48000, mode="s", bitrate=64, psy_model=1))
    assert t.down_feed is None and t.down_feed_stride == 0
    t.close()


def test_node_routes_down_feeds_and_restores_them_on_a_restart(M):
    """devices = (0, 0): two shards; frames, reports and down_feed_want equal one tick object's; a restarted shard has its down feeds again
    at tick 0; the exclusions on the node; a BATCH-plane node sets the shard's batch and refuses down_feed_want"""
    from pcmgen import gen_pcm
    sh = A.shared()
    live = F.interleave(gen_pcm(977, 0, 0, A.NTICKS), 2)
    scfgs = A.stream_configs()
    nd = M.Node(scfgs, devices=(0, 0), plane="tick", egress="frames")
    t = M.Tick(scfgs, egress="frames", ngroups=2)
    first, n0 = M.node_partition(NS, 2)[0]
    assert first == 0 and 0 < n0 < NS
    with pytest.raises(M.ToolameError) as e:
        nd.set_down_feed(0, M.FeedConfig(22050, 64, 2))          # no pair
    assert e.value.code == 1
    A.set_down_feeds(nd); A.set_down_feeds(t)
    for x in (nd.enable_short_reads, lambda: nd.set_source(22050, 6), lambda: nd.set_down_source(48000, 6), lambda: nd.set_feed(6, M.FeedConfig(24000, 64, 2))):
        with pytest.raises(M.ToolameError) as e:
            x()
        assert e.value.code == 18

    def node_fill(f, tick_of):
        row = np.full((NS, 2 * N), TICK_POISON, dtype=np.int16)
        row[NS - 1] = live[f]
        nd.set_pcm(row)
        for s in FED:
            L, Mm = A.lm_of(A.STREAMS[s])
            assert nd.down_feed_want(s) == A.want(tick_of(s), L, Mm), (f, s)
            slot, ln = nd.down_feed(s), nd.down_feed_len(s)
            assert not ln.any()
            for j in range(nd.down_feed_want(s)):
                b, n = sh["lists"][s][tick_of(s)][j]
                slot[j, :len(b)] = np.frombuffer(b, dtype=np.uint8)
                ln[j] = n
    for f in range(3):
        node_fill(f, lambda s: f)
        tick_fill(t, f, live)
        nd.run(); t.run()
        for s in range(NS):
            assert nd.frame(s) == t.frame(s), (f, s)
            assert nd.down_feed_report(s).tobytes() == t.down_feed_report[s].tobytes(), (f, s)
    nd.shard_restart(0)                                          # block 0 starts again: its down feeds at tick 0, block 1 goes on at tick 3
    fresh = M.Tick(scfgs[:n0], egress="frames")
    A.set_down_feeds(fresh, A.STREAMS[:n0])
    for k in range(3):
        node_fill(3 + k, lambda s: k if s < n0 else 3 + k)
        tick_fill(t, 3 + k, live)
        fresh.pcm[:] = TICK_POISON
        for s in range(n0):
            assert fresh.down_feed_want(s) == A.want(k, *A.lm_of(A.STREAMS[s]))
            for j in range(fresh.down_feed_want(s)):
                b, n = sh["lists"][s][k][j]
                fresh.down_feed[s, j, :len(b)] = np.frombuffer(b, dtype=np.uint8)
                fresh.down_feed_len[s, j] = n
        nd.run(); t.run(); fresh.run()
        for s in range(NS):
            x, i = (fresh, s) if s < n0 else (t, s)
            assert nd.frame(s) == x.frame(i), (k, s)
            assert nd.down_feed_report(s).tobytes() == x.down_feed_report[i].tobytes(), (k, s)
    nd.close(); t.close(); fresh.close()
    other = M.Node(scfgs, devices=(0, 0), plane="tick", egress="frames")
    other.set_down_source(48000, 6)
    with pytest.raises(M.ToolameError) as e:                     # ... from the other side
        other.set_down_feed(0, A.feed_config(A.STREAMS[0]))
    assert e.value.code == 18 and other.down_feed(0) is None
    other.close()
    nb = M.Node(scfgs, devices=(0, 0), plane="batch")
    nb.set_down_feed(0, A.feed_config(A.STREAMS[0]))             # tlb_feed_down_set of the shard's batch
    with pytest.raises(M.ToolameError) as e:
        nb.down_feed_want(0)
    assert e.value.code == 18
    nb.close()
