"""Layer II feeds on the device (tlb_feed_*): bit for bit against the lane-loop emulation of the same kernel source on a mixed batch, the
transcode chain feed -> ingest -> encode against a plain batch given the PCM tlb_decode_* makes of the same source frames, and the
batch-level rules (what a feed must fit, removal, resets, reconfiguration, a stride that grows between calls).  Source frames come from a
second Batch with the feed's configuration."""
import numpy as np
import pytest

import declib as D
import feedlib as F

pytestmark = pytest.mark.gpu

UNFED = [(48000, "s", 128), (48000, "m", 64), (24000, "s", 64)]  # streams 8..10 of the mixed batch: PCM input


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def feed_so(tmp_path_factory):
    return F.build_emu(tmp_path_factory.mktemp("feedemu"))


def _scfg(M, fs, mode, kbps):
    return M.StreamConfig(samplerate=fs, mode=mode, bitrate=kbps, psy_model=1, pad_len=0)


@pytest.fixture(scope="module")
def source(M):
    """six frames per case from a Batch with the feeds' configurations: per stream the list of frames (encode, then the flushed last one)"""
    b = M.Batch([_scfg(M, fs, mode, kbps) for fs, mode, kbps, _ in F.CASES])
    pcm = np.stack([F.case_pcm(i, c) for i, c in enumerate(F.CASES)], axis=1)
    data, _ = b.encode(pcm)
    last = b.flush()
    b.close()
    frames = [D.cut_frames(data[s] + last[s], dict(samplerate=c[0], kbps=c[2])) for s, c in enumerate(F.CASES)]
    assert all(len(f) == F.NFRAMES for f in frames)
    assert {x[3] >> 6 for x in frames[1]} == {0, 1}              # the joint-stereo source does switch between stereo and joint stereo
    return frames


def mixed_batch(M, source):
    """12 streams: the eight cases (stream s fed with case s; the encoder's own bitrate is another one where the table has one), three
    streams without a feed, and case 0's frames without their CRC-16 on a stream of its own"""
    other = {192: 128, 128: 192, 64: 96, 384: 192, 32: 48}
    scfgs = [_scfg(M, fs, mode, other[kbps]) for fs, mode, kbps, _ in F.CASES] + [_scfg(M, *u) for u in UNFED] + [_scfg(M, 48000, "j", 160)]
    fcfgs = [F.feed_cfg_of(c) for c in F.CASES] + [None] * len(UNFED) + [F.feed_cfg_of(F.CASES[0])]
    lists = list(source) + [[] for _ in UNFED] + [[F.strip_crc(x) for x in source[0]]]
    b = M.Batch(scfgs)
    for s, fc in enumerate(fcfgs):
        if fc:
            b.set_feed(s, M.FeedConfig(**fc))
    return b, fcfgs, lists


@pytest.fixture(scope="module")
def mixed_run(M, feed_so, source):
    """test 1's device run, kept for the tests that compare with it"""
    b, fcfgs, lists = mixed_batch(M, source)
    stride = b.feed_stride
    assert stride == 1728 == max(F.slot_bytes(c) for c in fcfgs if c)
    fr, ln = D.batch_arrays(lists, stride)
    assert fr.shape[0] == F.NFRAMES and not ln[:, 8:11].any()
    init = np.random.default_rng(3).integers(-32768, 32768, (F.NFRAMES, len(fcfgs), 2304)).astype(np.int16)
    parts = [b.feed(fr[:2], ln[:2], init[:2]), b.feed(fr[2:], ln[2:], init[2:])]      # cut 2 + 4
    got = tuple(np.concatenate([p[k] for p in parts]) for k in range(2))
    b.close()
    e = F.FeedEmu(feed_so, fcfgs)
    assert e.stride == stride
    want = e.decode(fr, ln, init)
    e.close()
    return dict(fcfgs=fcfgs, fr=fr, ln=ln, init=init, got=got, want=want)


def test_device_equals_emulation_on_a_mixed_batch(mixed_run):
    """Test 1.  PCM and reports of the device are the emulation's, bit for bit; the slots of streams without a feed, and what lies behind a
    one-channel feed's 1152 samples, are byte-identical to what was in the buffer."""
    r = mixed_run
    pcm, rep = r["got"]
    assert pcm.tobytes() == r["want"][0].tobytes()
    assert rep.tobytes() == r["want"][1].tobytes()
    w = F.expected_written(pcm, r["fcfgs"])
    assert np.array_equal(pcm[~w], r["init"][~w]) and w[:, 8:11].sum() == 0
    fed = [s for s, c in enumerate(r["fcfgs"]) if c]
    assert not rep["status"][:, fed].any() and (rep["status"][:, 8:11] == D.EMPTY).all()
    assert np.array_equal(pcm[:, 11], pcm[:, 0])                 # the same audio without its CRC-16
    for s in fed:
        assert np.abs(pcm[:, s, :1152].astype(int)).max() > 1000, s


def test_transcode_chain_equals_a_plain_batch_on_the_decoded_pcm(M, source):
    """Test 2.  feed -> ingest -> encode gives byte-identical output frames to a plain batch given the PCM the existing Batch.decode made
    of the same source frames."""
    src_cfgs = [_scfg(M, fs, mode, kbps) for fs, mode, kbps, _ in F.CASES]
    out_cfgs = [_scfg(M, fs, "j" if mode in "sj" else mode, 128 if fs >= 32000 and mode != "m" else 64) for fs, mode, _, _ in F.CASES]
    d = M.Batch(src_cfgs)
    fr, ln = D.batch_arrays(source, d.out_stride)
    rep, _, planar = d.decode(fr, ln, False, True)
    d.close()
    assert not (rep["status"] & D.BAD_MASK).any() and np.abs(planar.astype(int)).max() > 1000
    plain = M.Batch(out_cfgs)
    want, _ = plain.encode(planar)
    want_last = plain.flush()
    plain.close()
    b = M.Batch(out_cfgs)
    for s, c in enumerate(F.CASES):
        b.set_feed(s, M.FeedConfig(**F.feed_cfg_of(c)))
    ffr, fln = D.batch_arrays(source, b.feed_stride)
    inter, frep = b.feed(ffr, fln)
    assert not frep["status"].any()
    pcm, _ = b.ingest(inter)
    assert np.array_equal(pcm, planar)
    got, _ = b.encode(pcm)
    got_last = b.flush()
    b.close()
    assert got == want and got_last == want_last and all(len(x) > 0 for x in got)


def test_what_a_feed_must_fit(M):
    """the feed's rate and channel count must be the stream's; an illegal configuration is refused with its own code; nothing changes"""
    b = M.Batch([_scfg(M, 48000, "s", 128), _scfg(M, 48000, "m", 64), _scfg(M, 24000, "j", 64)])
    assert b.feed_stride == 0 and b.get_feed(0) is None
    for stream, cfg, code in ((0, M.FeedConfig(44100, 128, 2), 1), (0, M.FeedConfig(48000, 128, 1), 2), (1, M.FeedConfig(48000, 64, 2), 2),
                              (2, M.FeedConfig(48000, 64, 2), 1), (-1, M.FeedConfig(48000, 128, 2), 2), (0, M.FeedConfig(48000, 100, 2), 4),
                              (0, M.FeedConfig(48000, 128, 3), 2), (3, M.FeedConfig(48000, 128, 2), 18), (-2, None, 18)):
        with pytest.raises(M.ToolameError) as e:
            b.set_feed(stream, cfg)
        assert e.value.code == code, (stream, cfg)
        assert b.feed_stride == 0 and all(b.get_feed(s) is None for s in range(3))
    with pytest.raises(M.ToolameError) as e:                     # no stream has a feed: nothing to decode
        b.feed(np.zeros((1, 3, 0), dtype=np.uint8), np.zeros((1, 3), dtype=np.int32))
    assert e.value.code == 18
    b.set_feed(0, M.FeedConfig(48000, 192, 2))
    assert b.feed_stride == 576 and b.get_feed(0) == M.FeedConfig(48000, 192, 2)
    b.set_feed(2, M.FeedConfig(24000, 160, 2))
    assert b.feed_stride == 960
    b.set_feed(2, None)
    assert b.feed_stride == 576 and b.get_feed(2) is None
    b.stream_reconfigure(0, _scfg(M, 48000, "d", 96))            # still two channels at 48 kHz: the feed stays
    assert b.get_feed(0) == M.FeedConfig(48000, 192, 2)
    b.stream_reconfigure(0, _scfg(M, 48000, "m", 96))            # one channel now: the feed no longer fits and is removed
    assert b.get_feed(0) is None and b.feed_stride == 0
    b.close()


def test_history_removal_resets_and_a_growing_stride(M, source, mixed_run):
    """one stream's frames in two calls with, in between: another stream gaining a longer feed (the stride grows, the history is kept), a
    stream_reset of a third (its next frame is decoded as after silence) and the removal of a fourth's feed (its slots are PCM again)"""
    fc = F.feed_cfg_of(F.CASES[0])
    one = mixed_run["got"][0][:, 0]                              # case 0 decoded in the mixed batch
    b = M.Batch([_scfg(M, 48000, "s", 128)] * 4 + [_scfg(M, 32000, "s", 128)])
    for s in range(4):
        b.set_feed(s, M.FeedConfig(**fc))
    assert b.feed_stride == 576
    lists = [source[0]] * 4 + [[]]
    fr, ln = D.batch_arrays([x[:2] for x in lists[:4]] + [[b"", b""]], 576)
    a, _ = b.feed(fr, ln)
    b.set_feed(4, M.FeedConfig(**F.feed_cfg_of(F.CASES[5])))     # 32 kHz 384 kbps: 1728-byte slots
    assert b.feed_stride == 1728
    b.stream_reset(1)
    b.feed_reset(2)
    b.set_feed(3, None)
    fr, ln = D.batch_arrays([x[2:] for x in lists[:4]] + [source[5][2:]], 1728)
    init = np.full((4, 5, 2304), F.POISON, dtype=np.int16)
    c, rep = b.feed(fr, ln, init)
    b.close()
    assert np.array_equal(np.concatenate([a[:, 0], c[:, 0]]), one)
    for s in (1, 2):                                             # as after silence: the first frame differs, the rest is the same again
        assert not np.array_equal(c[0, s], one[2]) and np.array_equal(c[1:, s], one[3:])
        assert np.array_equal(c[:, s], c[:, 1])
    assert (c[:, 3] == F.POISON).all() and (rep["status"][:, 3] == D.EMPTY).all()
    assert np.array_equal(c[1:, 4], mixed_run["got"][0][3:, 5]) and not rep["status"][:, [0, 1, 2, 4]].any()


# ---- the tick plane ------------------------------------------------------------------------------------------------------------------
# eight streams in two groups of four: group 0 all fed (its PCM is not copied in), group 1 mixed.  (case fed or None, the encoder's mode and
# bitrate); rates whose frames are whole EDI units only.
TICK_STREAMS = [(0, "j", 128), (1, "s", 192), (3, "m", 96), (6, "m", 64), (2, "d", 128), (None, "s", 128), (7, "j", 64), (None, "m", 64)]
TICK_RATES = [48000, 48000, 48000, 24000, 48000, 48000, 16000, 48000]
NTICKS = 5
TICK_POISON = 0x5A5A


def tick_setup(M, source):
    scfgs = [_scfg(M, fs, mode, kbps) for fs, (_, mode, kbps) in zip(TICK_RATES, TICK_STREAMS)]
    fcfgs = [None if c is None else F.feed_cfg_of(F.CASES[c]) for c, _, _ in TICK_STREAMS]
    assert all(fc is None or fc["samplerate"] == fs for fc, fs in zip(fcfgs, TICK_RATES))
    lists = [[] if c is None else source[c][:NTICKS] for c, _, _ in TICK_STREAMS]
    from pcmgen import gen_pcm
    live = {s: F.interleave(gen_pcm(900 + s, 0, 0, NTICKS), 1 if TICK_STREAMS[s][1] == "m" else 2) for s in (5, 7)}      # the PCM of the unfed streams
    return scfgs, fcfgs, lists, live


def fill(t, f, fcfgs, lists, live, fed=None):
    """tick f's input: feed frames for the fed streams (poison in their PCM slots), PCM for the others"""
    fed = [c is not None for c in fcfgs] if fed is None else fed
    pcm = t.pcm
    pcm[:] = TICK_POISON
    for s in live:
        pcm[s] = live[s][f]
    fr, ln = t.feed, t.feed_len
    assert fr is not None and fr.shape == (len(fcfgs), t.feed_stride) and not ln.any()
    for s, on in enumerate(fed):
        if on:
            b = lists[s][f]
            fr[s, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            ln[s] = len(b)


def snap(t, egress, n):
    return [(t.frame(s) if egress == "frames" else t.packets(s), tuple(int(x) for x in t.peaks[s])) for s in range(n)]


@pytest.mark.parametrize("egress", ["frames", "af"])
def test_tick_with_feeds_equals_tick_given_the_decoded_pcm(M, source, egress):
    """Test 3.  Five ticks overlapped submit / submit / wait: frames (or AF packets) and peaks equal a tick object given the PCM the batch
    level decodes from the same frames; feed_report equals the batch level's reports; the all-feed group's PCM buffer holds poison."""
    scfgs, fcfgs, lists, live = tick_setup(M, source)
    n = len(scfgs)
    r = M.Batch(scfgs)
    for s, fc in enumerate(fcfgs):
        if fc:
            r.set_feed(s, M.FeedConfig(**fc))
    fr, ln = D.batch_arrays([x if x else [b""] * NTICKS for x in lists], r.feed_stride)
    init = np.zeros((NTICKS, n, 2304), dtype=np.int16)
    for s in live:
        init[:, s] = live[s]
    want_pcm, want_rep = r.feed(fr, ln, init)
    stride = r.feed_stride
    r.close()
    kw = dict(egress=egress, ngroups=2, version=b"fd", now_s=1712345678, delay_ms=370, tist=True)
    a, b = M.Tick(scfgs, **kw), M.Tick(scfgs, **kw)
    assert a.feed is None and a.feed_report is None and a.feed_stride == 0
    for s, fc in enumerate(fcfgs):
        if fc:
            a.set_feed(s, M.FeedConfig(**fc))
    assert a.feed_stride == stride == 576
    got, exp, reps = [], [], []

    def submit(f):
        fill(a, f, fcfgs, lists, live)
        b.pcm[:] = want_pcm[f]
        a.submit(); b.submit()

    def wait():
        a.wait(); b.wait()
        got.append(snap(a, egress, n)); exp.append(snap(b, egress, n)); reps.append(a.feed_report.copy())
    submit(0); submit(1)
    assert a.feed is None and a.feed_len is None                 # two ticks in flight: no input set is free
    wait()
    for f in range(2, NTICKS):
        submit(f); wait()
    wait()
    a.finish(); b.finish()
    got.append(snap(a, egress, n)); exp.append(snap(b, egress, n))
    assert len(got) == NTICKS + 1
    for f in range(NTICKS + 1):
        for s in range(n):
            assert got[f][s] == exp[f][s], (f, s)
        if f >= 1:
            assert all(len(x[0]) > 0 for x in got[f])
    assert np.array_equal(np.stack(reps), want_rep)
    assert np.array_equal(a.feed_report, want_rep[-1])            # the flush runs no feed kernel: the last tick's reports once more
    assert not want_rep["status"][:, [s for s, c in enumerate(fcfgs) if c]].any() and (want_rep["status"][:, [5, 7]] == D.EMPTY).all()
    a.close(); b.close()


def test_tick_without_a_feed_is_what_it_was(M, source):
    """an object that never sets a feed (or removes one it never had, or sets one and removes it again): its frames and peaks equal the
    stage-by-stage path on the same input (ingest, encode).  What it computes is checked; which device calls it queues is the submit's
    branch on the groups' any_fed."""
    scfgs, fcfgs, lists, live = tick_setup(M, source)
    n = len(scfgs)
    from pcmgen import gen_pcm
    inter = np.stack([F.interleave(gen_pcm(700 + s, 0, 0, NTICKS), 1 if TICK_STREAMS[s][1] == "m" else 2) for s in range(n)], axis=1)
    b = M.Batch(scfgs)
    pcm, peaks = b.ingest(inter)
    lens = np.zeros((NTICKS, n), dtype=np.int32)
    frames = np.zeros((NTICKS, n, b.out_stride), dtype=np.uint8)
    assert b.L.tlb_encode_host_len(b.h, pcm.ctypes.data, NTICKS, None, None, frames.ctypes.data, lens.ctypes.data, None) == 0
    b.close()
    plain = M.Tick(scfgs, egress="frames", ngroups=2)            # never touched by any feed call
    t = M.Tick(scfgs, egress="frames", ngroups=2)
    t.set_feed(-1, None)                                         # "off" on an object that never had one: nothing happens
    t.set_feed(0, M.FeedConfig(**fcfgs[0])); t.set_feed(0, None)  # on and off again: no feed is set
    assert t.feed is None and t.feed_len is None and t.feed_report is None and t.feed_stride == 0
    t.enable_short_reads()                                       # ... so short reads are not refused
    assert plain.feed is None and plain.feed_len is None and plain.feed_report is None and plain.feed_stride == 0
    for f in range(NTICKS):
        for x in (plain, t):
            x.pcm[:] = inter[f]
            x.run()
            assert np.array_equal(x.peaks, peaks[f])
            for s in range(n):
                assert x.frame(s) == frames[f, s, :lens[f, s]].tobytes(), (f, s)
    plain.close(); t.close()


def test_tick_feed_rules(M, source):
    """Test 4.  Feeds exclude short reads and sources, from either side; what a feed must fit; no set while a tick is in flight."""
    scfgs, fcfgs, lists, live = tick_setup(M, source)
    fc0 = M.FeedConfig(**fcfgs[0])
    t = M.Tick(scfgs, egress="frames", ngroups=2)
    t.enable_short_reads()
    with pytest.raises(M.ToolameError) as e:
        t.set_feed(0, fc0)
    assert e.value.code == 18 and t.feed is None
    t.set_feed(0, None)                                          # removing what is not there is no feed
    t.close()
    t = M.Tick(scfgs, egress="frames", ngroups=2)
    t.set_feed(0, fc0)
    with pytest.raises(M.ToolameError) as e:
        t.enable_short_reads()
    assert e.value.code == 18 and t.valid is None
    with pytest.raises(M.ToolameError) as e:
        t.set_source(44100, 1)
    assert e.value.code == 18 and t.need(1) == 1152
    for stream, cfg, code in ((3, fc0, 1), (2, fc0, 2), (-1, fc0, 2), (0, M.FeedConfig(48000, 100, 2), 4), (8, fc0, 18)):
        with pytest.raises(M.ToolameError) as e:
            t.set_feed(stream, cfg)
        assert e.value.code == code, (stream, cfg)
    assert t.feed_stride == 576
    t.pcm[:] = 0
    t.submit()
    with pytest.raises(M.ToolameError) as e:                     # a tick is in flight
        t.set_feed(1, fc0)
    assert e.value.code == 18
    t.wait()
    t.set_feed(1, M.FeedConfig(48000, 384, 2))                   # a wider feed: the buffers are replaced
    assert t.feed_stride == 1152 and t.feed.shape == (8, 1152)
    t.close()
    u = M.Tick(scfgs, egress="frames", ngroups=2)
    u.set_source(44100, 0)
    with pytest.raises(M.ToolameError) as e:
        u.set_feed(1, fc0)
    assert e.value.code == 18 and u.feed is None
    u.close()


def test_tick_feed_removal_and_stream_reset(M, source):
    """Test 4, second half.  Between ticks: stream_reset of a fed stream (its next frame is decoded as after silence), a feed removed (the
    stream takes PCM again, its all-feed group becomes a mixed one) and set again (fresh history).  The reference is a tick object given the
    PCM a Batch decodes under the same calls."""
    scfgs, fcfgs, lists, live = tick_setup(M, source)
    n = len(scfgs)
    from pcmgen import gen_pcm
    extra = F.interleave(gen_pcm(77, 0, 0, NTICKS), 2)           # stream 1's PCM while it has no feed
    r = M.Batch(scfgs)
    a, b = M.Tick(scfgs, egress="frames", ngroups=2), M.Tick(scfgs, egress="frames", ngroups=2)
    for s, fc in enumerate(fcfgs):
        if fc:
            r.set_feed(s, M.FeedConfig(**fc)); a.set_feed(s, M.FeedConfig(**fc))
    fed = [c is not None for c in fcfgs]
    for f in range(NTICKS):
        if f == 2:
            for x in (r, a, b):
                x.stream_reset(0)
            r.set_feed(1, None); a.set_feed(1, None)
            fed[1] = False
        if f == 4:
            r.set_feed(1, M.FeedConfig(**fcfgs[1])); a.set_feed(1, M.FeedConfig(**fcfgs[1]))
            fed[1] = True
        src = dict(live)
        if not fed[1]:
            src[1] = extra
        fill(a, f, fcfgs, lists, src, fed)
        fr, ln = F.slots_to_arrays([[(lists[s][f], len(lists[s][f])) if fed[s] else (b"", 0)] for s in range(n)], r.feed_stride)
        init = np.zeros((1, n, 2304), dtype=np.int16)
        for s in src:
            init[0, s] = src[s][f]
        want_pcm, want_rep = r.feed(fr, ln, init)
        b.pcm[:] = want_pcm[0]
        a.run(); b.run()
        assert np.array_equal(a.feed_report, want_rep[0]) and np.array_equal(a.peaks, b.peaks)
        for s in range(n):
            assert a.frame(s) == b.frame(s), (f, s)
    assert all(len(a.frame(s)) > 0 for s in range(n))
    a.close(); b.close(); r.close()


# ---- the node plane ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("egress", ["frames", "af"])
def test_node_with_feeds_either_side_of_the_cut_equals_one_tick_object(M, source, egress):
    """Test 5.  devices = {0, 0}: two shards of four streams; feeds on streams 3 and 4, the two either side of the cut, the rest PCM.  Frames,
    packets, peaks and feed reports equal one tick object's under the same calls; the accessors answer None where a shard has no feed; a
    restarted shard gets its feed again, with fresh history, as a fresh object's."""
    scfgs, fcfgs, lists, _ = tick_setup(M, source)
    n = len(scfgs)
    fed = [s in (3, 4) for s in range(n)]
    from pcmgen import gen_pcm
    live = {s: F.interleave(gen_pcm(300 + s, 0, 0, NTICKS), 1 if TICK_STREAMS[s][1] == "m" else 2) for s in range(n) if not fed[s]}
    kw = dict(egress=egress, version=b"fd", now_s=1712345678, tist=True)
    nd = M.Node(scfgs, devices=(0, 0), plane="tick", **kw)
    t = M.Tick(scfgs, ngroups=2, **kw)
    blocks = M.node_partition(n, 2)
    assert blocks == [(0, 4), (4, 4)]
    assert nd.feed(3) is None and nd.feed_len(3) is None and nd.feed_report(3) is None
    for s in (3, 4):
        nd.set_feed(s, M.FeedConfig(**fcfgs[s])); t.set_feed(s, M.FeedConfig(**fcfgs[s]))
    with pytest.raises(M.ToolameError) as e:                     # what a feed must fit, through the node
        nd.set_feed(2, M.FeedConfig(**fcfgs[0]))
    assert e.value.code == 2
    with pytest.raises(M.ToolameError) as e:
        nd.enable_short_reads()
    assert e.value.code == 18
    with pytest.raises(M.ToolameError) as e:
        nd.set_source(44100, 0)
    assert e.value.code == 18

    def node_fill(f, frame_of):
        row = np.full((n, 2304), TICK_POISON, dtype=np.int16)
        for s in live:
            row[s] = live[s][f]
        nd.set_pcm(row)
        for s in (3, 4):
            b = lists[s][frame_of(s)]
            slot, ln = nd.feed(s), nd.feed_len(s)
            assert slot is not None and len(slot) >= len(b) and ln[0] == 0
            slot[:len(b)] = np.frombuffer(b, dtype=np.uint8)
            ln[0] = len(b)

    def same(s, x, k):
        assert nd.frame(s) == x.frame(k) and nd.packets(s) == x.packets(k) and tuple(nd.peaks(s)) == tuple(x.peaks[k]), s
    for f in range(3):
        node_fill(f, lambda s: f)
        fill(t, f, fcfgs, lists, live, fed)
        nd.run(); t.run()
        for s in range(n):
            same(s, t, s)
            assert nd.feed_report(s) == t.feed_report[s], (f, s)
        assert int(nd.feed_report(3)["status"]) == 0 and int(nd.feed_report(0)["status"]) == D.EMPTY
    nd.shard_restart(0)                                          # block 0 starts again (its feed on stream 3 with fresh history), block 1 goes on
    fresh = M.Tick(scfgs[:4], **kw)
    fresh.set_feed(3, M.FeedConfig(**fcfgs[3]))
    for k in range(2):
        node_fill(3 + k, lambda s: 3 + k)
        fill(t, 3 + k, fcfgs, lists, live, fed)
        fill(fresh, 3 + k, fcfgs[:4], lists[:4], {s: v for s, v in live.items() if s < 4}, fed[:4])
        nd.run(); t.run(); fresh.run()
        for s in range(n):
            same(s, fresh if s < 4 else t, s)
        assert nd.feed_report(3) == fresh.feed_report[3] and nd.feed_report(4) == t.feed_report[4]
    nd.set_feed(3, None)                                         # shard 0 has no feed left
    assert nd.feed(3) is None and nd.feed_report(3) is None and nd.feed(4) is not None
    nd.close(); t.close(); fresh.close()
    nb = M.Node(scfgs, devices=(0, 0), plane="batch")            # a BATCH-plane node: the feed goes to the shard's batch, the tick accessors answer nothing
    nb.set_feed(4, M.FeedConfig(**fcfgs[4]))
    assert nb.feed(4) is None and nb.feed_len(4) is None and nb.feed_report(4) is None
    nb.close()
    ns_ = M.Node(scfgs, devices=(0, 0), plane="tick", egress="frames")
    ns_.enable_short_reads()
    with pytest.raises(M.ToolameError) as e:
        ns_.set_feed(4, M.FeedConfig(**fcfgs[4]))
    assert e.value.code == 18
    ns_.close()


def test_a_refused_set_feed_leaves_no_feed_and_the_accepted_one_equals_the_twin(M, source):
    """tlb_tick_set_feed is all or nothing, as the other opt-ins are (tests/test_optin_atomic_gpu.py): the fault-injection build refuses the nth
    allocation of the library's memory owner for nth = 1, 2, ... until the call is accepted.  Every refused attempt answers TLB_ERR_HIP and
    leaves no stream with a feed and the object healthy; the object then produces the frames of a twin that set its feeds with nothing armed."""
    FI = M.load_fault_library()
    scfgs = [_scfg(M, 48000, "s", 128)] * 4
    fc = M.FeedConfig(**F.feed_cfg_of(F.CASES[0]))
    t, twin = M.Tick(scfgs, egress="frames", ngroups=2, lib=FI), M.Tick(scfgs, egress="frames", ngroups=2, lib=FI)
    twin.set_feed(-1, fc)
    refused = 0
    try:
        for nth in range(1, 65):
            assert FI.tlb_debug_alloc_fail_next(nth) == 0
            try:
                t.set_feed(-1, fc)
                break
            except M.ToolameError as e:
                assert e.code == 17, (nth, e.code)
            assert t.feed is None and t.feed_len is None and t.feed_report is None and t.feed_stride == 0 and t.status() == 0, nth
            refused += 1
        else:
            pytest.fail("not accepted")
    finally:
        FI.tlb_debug_alloc_fail_next(0)
    assert refused >= 4                                          # lengths and reports, the frame buffers, each group's batch
    for f in range(3):
        for x in (t, twin):
            b = source[0][f]
            x.feed[:, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            x.feed_len[:] = len(b)
            x.run()
        assert not t.feed_report["status"].any()
        for s in range(4):
            assert t.frame(s) == twin.frame(s) and (f == 0 or len(t.frame(s)) > 0), (f, s)
    t.close(); twin.close()
