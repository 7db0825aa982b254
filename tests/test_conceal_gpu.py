"""Feed concealment on the device (tlb_conceal_*; csrc/toolame_conceal.hip): the scenario batch of tests/conceallib.py against the oracle bit
for bit under four cuts into calls, the attenuation property on device output, the tick plane and a one-shard node against the batch
plane over twelve ticks with a drop pattern, and a batch that never enables concealment against the feed emulation."""
import numpy as np
import pytest

import conceallib as K
import declib as D
import feedlib as F

pytestmark = pytest.mark.gpu

GPU_CASES = [1, 3, 4]          # joint stereo, mono, 44.1 kHz with its padding slot; with the all-empty wide feed the slots are 1728 bytes


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def _scfg(M, fcfg):
    if fcfg is None:
        return M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1, pad_len=0)
    return M.StreamConfig(samplerate=fcfg["samplerate"], mode="m" if fcfg["channels"] == 1 else "s", bitrate=128 if fcfg["channels"] == 2 else 64, psy_model=1, pad_len=0)


def batch_of(M, rows):
    b = M.Batch([_scfg(M, r["fcfg"]) for r in rows])
    for s, r in enumerate(rows):
        if r["fcfg"]:
            b.set_feed(s, M.FeedConfig(**r["fcfg"]))
    for s, r in enumerate(rows):
        if r["hold"]:
            b.enable_conceal(r["hold"], r["step"], stream=s)
    return b


def run_cut(b, fr, ln, cut):
    at, pcm, rep = 0, [], []
    for n in cut:
        p, r = b.feed(fr[at:at + n], ln[at:at + n], np.full((n, fr.shape[1], 2304), K.POISON, dtype=np.int16))
        pcm.append(p); rep.append(r)
        at += n
    return np.concatenate(pcm), np.concatenate(rep), b.conceal_records()


@pytest.fixture(scope="module")
def scene(M):
    rows = K.scenario_batch(GPU_CASES)
    b = batch_of(M, rows)
    fr, ln = K.batch_arrays(rows, b.feed_stride)
    yield rows, b, fr, ln
    b.close()


@pytest.mark.parametrize("cut", ["12", "1", "3", "5+7"])
def test_the_scenario_batch_equals_the_oracle(scene, cut):
    """every PCM sample and every record word of every scenario stream; the fed stream without concealment is feedlib's numpy statement and
    the stream without a feed keeps what the buffer held.  One batch for all cuts: feed_reset between them starts every stream again."""
    rows, b, fr, ln = scene
    assert b.feed_stride == 1728 and len(rows) == len(GPU_CASES) * 18 + 2
    b.feed_reset()
    pcm, rep, rec = run_cut(b, fr, ln, K.CUTS[cut])
    K.check_rows(rows, pcm, rep, rec.view(K.RECORD_DTYPE), cut)


def test_a_repeat_is_the_good_frame_halved_per_step_of_three(M):
    """tests/test_conceal_emu.py's property on device output: |2^k y[i] - g[i]| <= 2^(k - 1) + 1 on samples 480..1151 of each channel"""
    case = K.CASES[0]
    fcfg = F.feed_cfg_of(case)
    frames = F.oracle_frames(case, F.case_pcm(0, case, K.NSLOTS) // 4)
    rows = [dict(fcfg=fcfg, hold=4, step=3), dict(fcfg=fcfg, hold=0, step=0)]
    good = [(x, len(x)) for x in frames]
    lossy = list(good)
    for f in (4, 5, 6, 7):
        lossy[f] = (b"", 0)
    b = batch_of(M, rows)
    fr, ln = F.slots_to_arrays([lossy, good], b.feed_stride)
    pcm, _ = b.feed(fr, ln)
    b.close()
    g = pcm[3, 1].astype(np.int64).reshape(1152, 2)
    assert np.array_equal(pcm[3, 0], pcm[3, 1]) and 1000 < np.abs(g).max() < 16384
    for k in (1, 2, 3, 4):
        y = pcm[3 + k, 0].astype(np.int64).reshape(1152, 2)
        d = np.abs((y[480:] << k) - g[480:])
        print(f"k = {k}: max |2^k y - g| = {int(d.max())}, bound {2 ** (k - 1) + 1}")
        assert d.max() <= 2 ** (k - 1) + 1 and np.abs(y[480:]).max() > 30, k


# ---- the tick plane and a one-shard node -------------------------------------------------------------------------------------------------
# four streams in two groups: case 0 with hold 4 / step 3, case 3 (mono) with hold 1 / step 21, case 0 without concealment, a PCM stream
PLANE_ROWS = [(0, 4, 3), (3, 1, 21), (0, 0, 0), (None, 0, 0)]
DROPS = {0: {3, 4, 7, 8, 9, 10, 11}, 1: {0, 5, 6, 7}, 2: {3, 4}}     # the ticks whose feed slot is empty


def plane_setup(M):
    rows = []
    for c, hold, step in PLANE_ROWS:
        fcfg = None if c is None else F.feed_cfg_of(K.CASES[c])
        frames = [] if c is None else K.case_frames(c)
        rows.append(dict(fcfg=fcfg, hold=hold, step=step, frames=frames))
    from pcmgen import gen_pcm
    live = F.interleave(gen_pcm(911, 0, 0, K.NSLOTS), 2)
    # the batch plane: one call per tick, the PCM the ingest is given and the records after every call
    b = batch_of(M, rows)
    want_pcm, want_rec = [], []
    for f in range(K.NSLOTS):
        slots = [[(r["frames"][f], len(r["frames"][f])) if r["fcfg"] and f not in DROPS[s] else (b"", 0)] for s, r in enumerate(rows)]
        fr, ln = F.slots_to_arrays(slots, b.feed_stride)
        init = np.zeros((1, 4, 2304), dtype=np.int16)
        init[0, 3] = live[f]
        want_pcm.append(b.feed(fr, ln, init)[0][0])
        want_rec.append(b.conceal_records())
    b.close()
    assert int(want_rec[-1][0]["muted"]) == 0 and int(want_rec[-1][0]["concealed"]) == 7 and int(want_rec[-1][1]["muted"]) == 2
    return rows, live, want_pcm, want_rec


def test_tick_and_node_equal_the_batch_plane(M):
    """twelve ticks with a drop pattern: the frames of a tick object with feeds and concealment, and of a node of one shard, equal those of a
    tick object given the PCM the batch plane made; their records equal the batch plane's after every tick"""
    rows, live, want_pcm, want_rec = plane_setup(M)
    scfgs = [_scfg(M, r["fcfg"]) for r in rows]
    kw = dict(egress="af", version=b"cc", now_s=1712345678, tist=True)
    a, ref = M.Tick(scfgs, ngroups=2, **kw), M.Tick(scfgs, ngroups=2, **kw)
    nd = M.Node(scfgs, devices=(0,), plane="tick", **kw)
    assert a.conceal() is None and nd.conceal(0) is None
    for x in (a, nd):
        with pytest.raises(M.ToolameError) as e:                 # no feed yet
            x.enable_conceal(4, 3, stream=0)
        assert e.value.code == 18
        for s, r in enumerate(rows):
            if r["fcfg"]:
                x.set_feed(s, M.FeedConfig(**r["fcfg"]))
        with pytest.raises(M.ToolameError) as e:                 # stream 3 has no feed: nothing is enabled
            x.enable_conceal(4, 3, stream=-1)
        assert e.value.code == 18
        for s, r in enumerate(rows):
            if r["hold"]:
                x.enable_conceal(r["hold"], r["step"], stream=s)
    assert a.conceal() is not None and not a.conceal().view(np.uint8).any()
    for f in range(K.NSLOTS):
        a.pcm[:] = 0x5A5A
        a.pcm[3] = live[f]
        row = np.full((4, 2304), 0x5A5A, dtype=np.int16)
        row[3] = live[f]
        nd.set_pcm(row)
        for s, r in enumerate(rows):
            if r["fcfg"] and f not in DROPS[s]:
                x = r["frames"][f]
                a.feed[s, :len(x)] = np.frombuffer(x, dtype=np.uint8)
                a.feed_len[s] = len(x)
                nd.feed(s)[:len(x)] = np.frombuffer(x, dtype=np.uint8)
                nd.feed_len(s)[0] = len(x)
        ref.pcm[:] = want_pcm[f]
        a.run(); ref.run(); nd.run()
        assert np.array_equal(a.peaks, ref.peaks), f
        for s in range(4):
            assert a.packets(s) == ref.packets(s) == nd.packets(s), (f, s)
            assert f == 0 or len(a.packets(s)) > 0
            assert nd.conceal(s) == want_rec[f][s], (f, s)
        assert a.conceal().tobytes() == want_rec[f].tobytes(), f
    a.conceal_reset(0); nd.conceal_reset(0)
    a.set_feed(1, M.FeedConfig(**rows[1]["fcfg"]))               # a feed set again: its concealment is off, the record starts again
    a.pcm[:] = 0; a.run()
    nd.set_pcm(np.zeros((4, 2304), dtype=np.int16)); nd.run()
    rec = a.conceal()
    assert [int(rec[s]["frames"]) for s in range(4)] == [1, 0, 0, 0] and int(rec[0]["muted"]) == 1
    assert int(nd.conceal(0)["frames"]) == 1 and int(nd.conceal(1)["frames"]) == K.NSLOTS + 1
    nd.shard_restart(0)                                          # the shard's streams get their feeds and their concealment again, from zero
    nd.set_pcm(np.zeros((4, 2304), dtype=np.int16)); nd.run()
    assert [(int(nd.conceal(s)["frames"]), int(nd.conceal(s)["muted"])) for s in range(4)] == [(1, 1), (1, 1), (0, 0), (0, 0)]
    a.close(); ref.close(); nd.close()


def test_a_batch_that_never_enables_it_is_the_feed_as_before(M, tmp_path):
    """the "ways" losses of case 0 on a batch that makes no concealment call: PCM and reports are the feed emulation's, bit for bit, there
    are no records to read and no stream has parameters"""
    rows = [r for r in K.scenario_batch([0]) if r["name"] in ("ways", "unconcealed", "wide", "unfed")]
    b = M.Batch([_scfg(M, r["fcfg"]) for r in rows])
    for s, r in enumerate(rows):
        if r["fcfg"]:
            b.set_feed(s, M.FeedConfig(**r["fcfg"]))
    fr, ln = K.batch_arrays(rows, b.feed_stride)
    init = np.full((K.NSLOTS, len(rows), 2304), K.POISON, dtype=np.int16)
    pcm, rep = b.feed(fr, ln, init)
    assert all(b.conceal_cfg(s) is None for s in range(len(rows)))
    with pytest.raises(M.ToolameError) as e:
        b.conceal_records()
    assert e.value.code == 18
    b.close()
    e = F.FeedEmu(F.build_emu(tmp_path), [r["fcfg"] for r in rows])
    want_pcm, want_rep = e.decode(fr, ln, init)
    e.close()
    assert pcm.tobytes() == want_pcm.tobytes() and rep.tobytes() == want_rep.tobytes()
    assert np.array_equal(pcm[:, 0], pcm[:, 1]) and not pcm[np.array(rows[0]["lost"]), 0].any()
