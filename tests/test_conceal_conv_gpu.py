"""Feed concealment on adapted and down feeds on the device (tlb_feed_loss_enable; csrc/toolame_conceal_conv.hip): the scenario batches of
tests/concealconvlib.py -- a few dozen streams over at most 23 ticks -- against the emulation and the oracle bit for bit under three cuts
into calls; the CHAIN on the device itself (a strict concealed batch at the feeds' own configuration, the channel map, Batch.resample or
Batch.decimate, against the converted concealed batch) for all seven feed cases; the tick plane and a one-shard node against the batch
plane with a drop pattern, their records behind the packets, a shard restart."""
import numpy as np
import pytest

import concealconvlib as V
import conceallib as K
import decimatelib as DC
import feedadaptlib as FA
import feeddownlib as FD
import feedlib as F
import resamplelib as R

pytestmark = pytest.mark.gpu

KINDS = {"adapt": [0, 1, 2, 3], "down": [4, 5, 6]}
NAMES = ("hold+1", "first", "alternating", "ways", "h16s1", "inside", "behind", "even", "unconcealed")


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def _scfg(M, rate, nch):
    return M.StreamConfig(samplerate=rate, mode="m" if nch == 1 else "s", bitrate=128 if rate >= 32000 and nch == 2 else 64, psy_model=1, pad_len=0)


def batch_of(M, rows):
    """the rows as a batch with their adapted or down feeds, concealment on through tlb_feed_loss_enable where a row has a hold"""
    kind = V.kind_of(rows)
    b = M.Batch([_scfg(M, r["enc_rate"], r["enc_nch"]) for r in rows])
    for s, r in enumerate(rows):
        if r["fcfg"]:
            if kind == "down":
                b.set_down_feed(s, M.FeedConfig(**r["fcfg"]))
            else:
                b.set_feed(s, M.FeedConfig(**r["fcfg"]), adapt=True)
    for s, r in enumerate(rows):
        if r["hold"]:
            b.enable_conceal(r["hold"], r["step"], stream=s, any_feed=True)
    return b


def run_cut(b, kind, fr, ln, cut):
    at, pcm, rep = 0, [], []
    for n in cut:
        init = np.full((n, fr.shape[1], 2304), V.POISON, dtype=np.int16)
        p, r = (b.down_feed if kind == "down" else b.feed)(fr[at:at + n], ln[at:at + n], init)
        pcm.append(p); rep.append(r)
        at += n
    assert at == fr.shape[0]
    return np.concatenate(pcm), np.concatenate(rep), b.conceal_records()


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_equals_emulation_equals_oracle(M, kind):
    """every PCM sample, report and record word of every scenario stream: the device's are the emulation's are the oracle's.  One batch for
    all cuts: the path's reset between them starts every stream again, its concealment included."""
    rows = V.multi_batch(KINDS[kind], NAMES)
    nt = len(rows[0]["ticks"])
    assert 30 <= len(rows) <= 40 and nt <= 24
    b = batch_of(M, rows)
    stride = b.down_feed_stride if kind == "down" else b.feed_stride
    fr, ln = V.batch_arrays(rows, stride)
    e = V.ConcealConvEmu(rows)
    assert e.stride == stride
    want = e.run_cut(fr, ln, [nt])
    assert e.guard_ok()
    e.close()
    V.check_rows(rows, want[0], want[1], want[2], "emulation")
    for cut in ([nt], [n for n in (5, 7, nt - 12) if n], [1] * nt):
        (b.down_feed_reset if kind == "down" else b.feed_reset)()
        pcm, rep, rec = run_cut(b, kind, fr, ln, cut)
        rec = rec.view(V.RECORD_DTYPE)
        V.check_rows(rows, pcm, rep, rec, str(cut))
        assert pcm.tobytes() == want[0].tobytes() and rep.tobytes() == want[1].tobytes() and rec.tobytes() == want[2].tobytes(), cut
    b.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_chain_on_the_device(M, kind):
    """the property the feature is defined by, with nothing but device code on either side: a STRICT feed at the feed's own rate and channel
    count with tlb_conceal_enable over the wanted slots, the channel map (numpy: (L + R + 1) >> 1, or one channel to both), then
    Batch.resample / Batch.decimate, equals the adapted or down feed with tlb_feed_loss_enable -- PCM bit for bit, and the records"""
    rows = [r for r in V.multi_batch(KINDS[kind], ("hold+1", "alternating", "inside")) if r["fcfg"] and r["hold"]]
    assert len(rows) == 3 * len(KINDS[kind])
    nt = len(rows[0]["ticks"])
    b = batch_of(M, rows)
    fr, ln = V.batch_arrays(rows, b.down_feed_stride if kind == "down" else b.feed_stride)
    got, _, rec = run_cut(b, kind, fr, ln, [nt])
    b.close()
    # the strict batch over every stream's wanted slots; a shorter sequence gets lost slots behind it (PCM before them does not depend on them)
    nw = max(len(r["wanted"]) for r in rows)
    strict = M.Batch([_scfg(M, r["fcfg"]["samplerate"], r["fcfg"]["channels"]) for r in rows])
    for s, r in enumerate(rows):
        strict.set_feed(s, M.FeedConfig(**r["fcfg"]))
        strict.enable_conceal(r["hold"], r["step"], stream=s)
    sf, sl = F.slots_to_arrays([list(r["wanted"]) + [(b"", 0)] * (nw - len(r["wanted"])) for r in rows], strict.feed_stride)
    src, _ = strict.feed(sf, sl)
    srec = strict.conceal_records()
    strict.close()
    # the map, and the slots Batch.resample / Batch.decimate take
    sigs, cfgs = [], []
    for s, r in enumerate(rows):
        fch = r["fcfg"]["channels"]
        x = src[:len(r["wanted"]), s, :1152 * fch].reshape(-1, fch)
        xm = np.ascontiguousarray(FA.channel_map(x, fch, r["enc_nch"])).astype(np.int16)
        sigs.append(xm)
        cfgs.append(dict(samplerate=r["enc_rate"], mode="m" if xm.shape[1] == 1 else "s", source=r["fcfg"]["samplerate"] if r["fcfg"]["samplerate"] != r["enc_rate"] else 0))
    if kind == "down":
        conv = M.Batch(DC.stream_configs(cfgs))
        for s, c in enumerate(cfgs):
            conv.set_down_source(c["source"], s)
        y = conv.decimate(DC.cut(sigs, cfgs, 0, nt))
    else:
        conv = M.Batch(R.stream_configs(cfgs))
        for s, c in enumerate(cfgs):
            if c["source"]:
                conv.set_source(c["source"], s)
        y = conv.resample(R.cut(sigs, cfgs, 0, nt))
    conv.close()
    for s, r in enumerate(rows):
        fch, sch = r["fcfg"]["channels"], r["enc_nch"]
        want = np.repeat(y[:, s, :1152], 2, axis=1) if fch == 1 and sch == 2 else y[:, s, :1152 * sch]
        bad = np.nonzero((got[:, s, :1152 * sch] != want).any(axis=1))[0]
        assert bad.size == 0, (V.CASE_IDS[r["ci"]], r["name"], "ticks", bad.tolist())
        assert got[:, s, :1152 * sch].any()
        if len(r["wanted"]) == nw:
            assert rec[s] == srec[s], (V.CASE_IDS[r["ci"]], r["name"])
        else:
            assert int(rec[s]["concealed"]) > 0


# ---- the tick plane and a one-shard node -------------------------------------------------------------------------------------------------
# per kind: (case or a strict feed, hold, step) per stream, then a PCM stream; the WANTED slots (counted per stream) that are lost
PLANES = {
    "adapt": dict(rows=[(1, 4, 3), (0, 1, 21), ("strict", 4, 3), (0, 0, 0), (None, 0, 0)], nticks=12,
                  drops={0: {3, 4, 7, 8, 9, 10}, 1: {0, 5, 6, 7}, 2: {2, 3, 9}, 3: {3, 4}}),
    "down": dict(rows=[(5, 4, 3), (4, 2, 5), (4, 0, 0), (None, 0, 0)], nticks=8,
                 drops={0: {2, 3, 4, 8}, 1: {1, 4, 5, 6, 7, 9}, 2: {3, 4}}),
}


def _plane_rows(M, kind):
    rows = []
    for c, hold, step in PLANES[kind]["rows"]:
        if c is None:
            rows.append(dict(fcfg=None, hold=0, step=0, frames=[], rate=24000 if kind == "down" else 48000, nch=2, strict=False))
        elif c == "strict":
            fc = F.feed_cfg_of(K.CASES[0])
            rows.append(dict(fcfg=fc, hold=hold, step=step, frames=K.case_frames(0), rate=fc["samplerate"], nch=fc["channels"], strict=True))
        else:
            case = V.CASES[c]
            rows.append(dict(fcfg=V.fcfg_of(case), hold=hold, step=step, frames=V.case_frames(c), rate=case[2][0], nch=V.enc_nch(case), strict=False))
    return rows


def _set_feeds(M, x, kind, rows):
    for s, r in enumerate(rows):
        if r["fcfg"]:
            fc = M.FeedConfig(**r["fcfg"])
            if kind == "down":
                x.set_down_feed(s, fc)
            else:
                x.set_feed(s, fc, adapt=not r["strict"])


def _tick_slots(kind, rows, drops, want_of, at):
    """the slots of one tick: per fed stream the next want_of(s) frames of its sequence, a dropped one left empty -> per stream a list of
    (slot j, bytes) to write"""
    out = []
    for s, r in enumerate(rows):
        put = []
        if r["fcfg"]:
            for j in range(want_of(s)):
                k = at[s]; at[s] += 1
                if k not in drops[s]:
                    put.append((j, r["frames"][k]))
        out.append(put)
    return out


@pytest.mark.parametrize("kind", list(PLANES))
def test_tick_and_node_equal_the_batch_plane(M, kind):
    """ticks with a drop pattern (a dropped frame is a wanted slot left empty): the frames of a tick object with adapted (or down) feeds
    and concealment, and of a node of one shard, equal those of a tick object given the PCM the batch plane made; their records equal the
    batch plane's after every tick; a restarted shard conceals again, from zero"""
    P = PLANES[kind]
    rows, drops, nticks = _plane_rows(M, kind), P["drops"], P["nticks"]
    ns = len(rows)
    scfgs = [_scfg(M, r["rate"], r["nch"]) for r in rows]
    from pcmgen import gen_pcm
    live = F.interleave(gen_pcm(911, 0, 0, nticks), 2)
    # the batch plane: one call per tick, the PCM the ingest is given and the records after every call
    b = M.Batch(scfgs)
    _set_feeds(M, b, kind, rows)
    for s, r in enumerate(rows):
        if r["hold"]:
            b.enable_conceal(r["hold"], r["step"], stream=s, any_feed=True)
    want_pcm, want_rec, plan, at = [], [], [], [0] * ns
    for f in range(nticks):
        put = _tick_slots(kind, rows, drops, (lambda s: b.down_feed_want(s)) if kind == "down" else (lambda s: b.feed_want(s)), at)
        plan.append(put)
        init = np.zeros((1, ns, 2304), dtype=np.int16)
        init[0, ns - 1] = live[f]
        if kind == "down":
            lists = [[[next(((x, len(x)) for j, x in put[s] if j == jj), (b"", 0)) for jj in range(2)]] for s in range(ns)]
            fr, ln = FD.slots_to_arrays(lists, b.down_feed_stride)
            want_pcm.append(b.down_feed(fr, ln, init)[0][0])
        else:
            lists = [[next(((x, len(x)) for j, x in put[s]), (b"", 0))] for s in range(ns)]
            fr, ln = F.slots_to_arrays(lists, b.feed_stride)
            want_pcm.append(b.feed(fr, ln, init)[0][0])
        want_rec.append(b.conceal_records())
    b.close()
    last = want_rec[-1]
    assert all(int(last[s]["concealed"]) > 0 for s, r in enumerate(rows) if r["hold"]) and int(last[1]["muted"]) > 0
    assert not last[[s for s, r in enumerate(rows) if not r["hold"]]].view(np.uint8).any()

    kw = dict(egress="af", version=b"cc", now_s=1712345678, tist=True)
    a, ref = M.Tick(scfgs, ngroups=2, **kw), M.Tick(scfgs, ngroups=2, **kw)
    nd = M.Node(scfgs, devices=(0,), plane="tick", **kw)
    for x in (a, nd):
        with pytest.raises(M.ToolameError) as e:                 # no feed yet
            x.enable_conceal(4, 3, stream=0, any_feed=True)
        assert e.value.code == 18
        _set_feeds(M, x, kind, rows)
        with pytest.raises(M.ToolameError) as e:                 # the strict call keeps refusing an adapted or a down feed
            x.enable_conceal(4, 3, stream=0)
        assert e.value.code == 18
        with pytest.raises(M.ToolameError) as e:                 # the last stream has no feed: nothing is enabled
            x.enable_conceal(4, 3, stream=-1, any_feed=True)
        assert e.value.code == 18
        for s, r in enumerate(rows):
            if r["hold"]:
                x.enable_conceal(r["hold"], r["step"], stream=s, any_feed=True)
    assert a.conceal() is not None and not a.conceal().view(np.uint8).any()
    at = [0] * ns
    for f in range(nticks):
        a.pcm[:] = 0x5A5A
        a.pcm[ns - 1] = live[f]
        row = np.full((ns, 2304), 0x5A5A, dtype=np.int16)
        row[ns - 1] = live[f]
        nd.set_pcm(row)
        for s, r in enumerate(rows):
            if not r["fcfg"]:
                continue
            w = a.down_feed_want(s) if kind == "down" else a.feed_want(s)
            assert w == (nd.down_feed_want(s) if kind == "down" else nd.feed_want(s)), (f, s)
            assert [j for j, _ in plan[f][s]] == [j for j in range(w) if at[s] + j not in drops[s]], (f, s)      # the batch plane's schedule
            at[s] += w
            for j, x in plan[f][s]:
                if kind == "down":
                    a.down_feed[s, j, :len(x)] = np.frombuffer(x, dtype=np.uint8)
                    a.down_feed_len[s, j] = len(x)
                    nd.down_feed(s)[j, :len(x)] = np.frombuffer(x, dtype=np.uint8)
                    nd.down_feed_len(s)[j] = len(x)
                else:
                    a.feed[s, :len(x)] = np.frombuffer(x, dtype=np.uint8)
                    a.feed_len[s] = len(x)
                    nd.feed(s)[:len(x)] = np.frombuffer(x, dtype=np.uint8)
                    nd.feed_len(s)[0] = len(x)
        ref.pcm[:] = want_pcm[f]
        a.run(); ref.run(); nd.run()
        assert np.array_equal(a.peaks, ref.peaks), f
        for s in range(ns):
            assert a.packets(s) == ref.packets(s) == nd.packets(s), (f, s)
            assert f == 0 or len(a.packets(s)) > 0
            assert nd.conceal(s) == want_rec[f][s], (f, s)
        assert a.conceal().tobytes() == want_rec[f].tobytes(), f
    # a feed set again: the stream's concealment is off and its record starts again; a restarted shard conceals again, from zero
    _set_feeds(M, a, kind, [r if s == 1 else dict(r, fcfg=None) for s, r in enumerate(rows)])
    a.pcm[:] = 0; a.run()
    rec = a.conceal()
    assert int(rec[1]["frames"]) == 0 and not rec[1].tobytes().strip(b"\0") and int(rec[0]["frames"]) >= int(want_rec[-1][0]["frames"])
    nd.shard_restart(0)
    nd.set_pcm(np.zeros((ns, 2304), dtype=np.int16)); nd.run()
    first = 2 if kind == "down" else 1                           # tick 0 of every schedule wants a full tick's slots; all are empty: lost, no G
    assert [(int(nd.conceal(s)["frames"]), int(nd.conceal(s)["muted"])) for s in range(ns)] == [(first, first) if r["hold"] else (0, 0) for r in rows]
    a.close(); ref.close(); nd.close()
