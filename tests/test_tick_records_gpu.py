"""Every record option of a tick object on at once (csrc/tlb_tick.cpp, tick_records: monitor, compare, loudness and true-peak records are
rows of one table, staged, copied out and read through one body each).  What a shared table can newly get wrong is one option's buffers,
event or size standing in for another's, so: object A has the AUDIO monitor, the compare monitor, the loudness meter and the true-peak meter
(with a ceiling that is not the default) all on and listens to a stream of the middle group.  Pipelined, tick by tick and at the finish,
A's packets are those of an object with nothing on, and each of A's four record arrays and the listened PCM are, byte for byte, those of an
object that enabled that option alone (the compare monitor needs the AUDIO monitor: its twin has both).  The same at node level with two
shards on one device, where shard 1 is restarted between steps: its streams answer through all four accessors again, and the true-peak
records of its streams are those of a fresh tick object with the node's ceiling."""
import numpy as np
import pytest

from pcmgen import gen_pcm

pytestmark = pytest.mark.gpu
NT = 5
LISTEN = 2                                                           # 3 groups over 5 streams: [0, 1) [1, 3) [3, 5) -- in the middle one
CEILING = 1 << 26                                                    # -24 dBTP: the tones (about -5 dBFS) are over it and under the default of -1 dBTP
RECORDS = ("monitor", "compare", "loudness", "truepeak")
# what each twin enables -> which of A's results it vouches for
TWINS = {"monitor": ("monitor", "pcm"), "monitor+compare": ("compare",), "loudness": ("loudness",), "truepeak": ("truepeak",)}


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def _cfgs(M):
    return [M.StreamConfig(mode="j", bitrate=128, psy_model=1)] * 3 + [M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1),
                                                                      M.StreamConfig(mode="m", bitrate=64, psy_model=1)]


@pytest.fixture(scope="module")
def pcm():
    """interleaved int16 [NT][5 streams][2304], seeded; shared and read-only"""
    a = np.stack([np.stack([gen_pcm(70 + s, 0, 0, NT)[f].T.reshape(-1) for s in range(5)]) for f in range(NT)])
    a.setflags(write=False)
    return a


def _enable(o, what, listen):
    """what: "" (nothing), "all", or one key of TWINS"""
    if what in ("all", "monitor", "monitor+compare"):
        o.enable_monitor("audio")
        o.monitor_listen(listen)
    if what in ("all", "monitor+compare"):
        o.enable_compare()
    if what in ("all", "loudness"):
        o.enable_loudness()
    if what in ("all", "truepeak"):
        o.enable_truepeak(CEILING)


def _pipelined(fill, o, frames, snap, out):
    """submit, submit, wait, submit, wait, ..., wait: one snapshot per waited tick, appended to out"""
    for i, f in enumerate(frames):
        fill(f)
        o.submit()
        if i:
            o.wait()
            out.append(snap())
    o.wait()
    out.append(snap())


def _tick_snap(t):
    b = lambda a: None if a is None else a.tobytes()
    s, p = t.monitor_pcm()
    return dict(packets=[t.packets(k) for k in range(t.nstreams)], monitor=b(t.monitor), compare=b(t.compare), loudness=b(t.loudness),
                truepeak=b(t.truepeak), pcm=(s, b(p)))


def _tick_play(M, pcm, what):
    t = M.Tick(_cfgs(M), egress="af", ngroups=3)
    _enable(t, what, LISTEN)
    out = []

    def fill(f):
        t.pcm[:] = pcm[f]
    _pipelined(fill, t, range(NT), lambda: _tick_snap(t), out)
    t.finish()
    out.append(_tick_snap(t))
    t.close()
    return out


def test_tick_with_every_record_option_on_equals_the_objects_that_have_one(M, pcm):
    a, plain = _tick_play(M, pcm, "all"), _tick_play(M, pcm, "")
    assert len(a) == NT + 1 and all(plain[f][k] is None for f in range(NT + 1) for k in RECORDS) and plain[NT]["pcm"] == (-1, None)
    for f in range(NT + 1):
        assert a[f]["packets"] == plain[f]["packets"], f
        assert all(a[f][k] is not None for k in RECORDS), f
    assert all(len(p) > 0 for p in a[NT]["packets"])                 # (the finish did hand out packets)
    assert [a[f]["pcm"][0] for f in range(NT + 1)] == [-1] + [LISTEN] * NT      # (the first tick has no frame to listen to)
    for what, keys in TWINS.items():
        twin = _tick_play(M, pcm, what)
        for f in range(NT + 1):
            for k in keys:
                assert a[f][k] == twin[f][k], (what, k, f)
    last = np.frombuffer(a[NT]["truepeak"], dtype=M.TRUEPEAK_DTYPE)
    assert (last["frames"] == NT).all() and (last["overs"][:3] > 0).all()      # (the meters ran on every tick; A's ceiling is the one given)
    assert (np.frombuffer(a[NT]["loudness"], dtype=M.LOUDNESS_DTYPE)["frames"] == NT).all()


def _node_snap(nd):
    b = lambda a: None if a is None else a.tobytes()
    s, p = nd.monitor_pcm()
    out = dict(packets=[nd.packets(k) for k in range(nd.nstreams)], pcm=(s, b(p)))
    for k in RECORDS:
        out[k] = [b(getattr(nd, k)(s)) for s in range(nd.nstreams)]
    return out


NODE_LISTEN, BEFORE = 3, 3                                           # a stream of shard 1; the restart comes after this many ticks


def _node_play(M, pcm, what):
    """BEFORE ticks, shard 1 restarted, the rest and the finish -> (the snapshots, the snapshot right after the restart)"""
    nd = M.Node(_cfgs(M), devices=(0, 0), plane="tick", egress="af", ngroups=2)
    _enable(nd, what, NODE_LISTEN)
    out = []
    fill = lambda f: nd.set_pcm(pcm[f])
    _pipelined(fill, nd, range(BEFORE), lambda: _node_snap(nd), out)
    nd.shard_restart(1)
    restarted = _node_snap(nd)
    _pipelined(fill, nd, range(BEFORE, NT), lambda: _node_snap(nd), out)
    nd.finish()
    out.append(_node_snap(nd))
    blocks = nd.blocks
    nd.close()
    return out, restarted, blocks


def test_node_with_every_record_option_on_and_a_restarted_shard(M, pcm):
    (a, a_restarted, blocks), (plain, _, _) = _node_play(M, pcm, "all"), _node_play(M, pcm, "")
    f1, n1 = blocks[1]
    mine = list(range(f1, f1 + n1))
    assert len(blocks) == 2 and NODE_LISTEN in mine and len(a) == NT + 1
    for f in range(NT + 1):
        assert a[f]["packets"] == plain[f]["packets"], f
        assert all(r is not None for k in RECORDS for r in a[f][k]), f
        assert all(r is None for k in RECORDS for r in plain[f][k]), f
    assert all(len(p) > 0 for p in a[NT]["packets"])
    assert all(a_restarted[k][s] is not None for k in RECORDS for s in mine)     # all four accessors answer for the restarted shard's streams
    assert all(a_restarted[k][s] == bytes(len(a_restarted[k][s])) for k in ("loudness", "truepeak") for s in mine)     # ... the meters from zero
    assert [a[f]["pcm"][0] for f in range(NT + 1)] == [-1] + [NODE_LISTEN] * (BEFORE - 1) + [-1] + [NODE_LISTEN] * (NT - BEFORE)      # (the listened stream is set again too)
    for what, keys in TWINS.items():
        twin, twin_restarted, _ = _node_play(M, pcm, what)
        for f in range(NT + 1):
            for k in keys:
                assert a[f][k] == twin[f][k], (what, k, f)
        for k in keys:
            assert a_restarted[k] == twin_restarted[k], (what, k)
    # the ceiling a restarted shard measures against is the node's: a fresh tick object over its streams, given that ceiling and the ticks since
    t = M.Tick(_cfgs(M)[f1:f1 + n1], egress="af", ngroups=1)
    t.enable_truepeak(CEILING)
    for f in range(BEFORE, NT):
        t.pcm[:] = pcm[f][f1:f1 + n1]
        t.run()
    want = t.truepeak.copy()
    t.close()
    assert (want["overs"] > 0).any()
    assert [a[NT]["truepeak"][s] for s in mine] == [want[i].tobytes() for i in range(n1)]
