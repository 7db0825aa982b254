"""The C-ABI of the feed concealment on adapted and down feeds (tlb_feed_loss_enable, tlb_tick_enable_feed_loss,
tlb_node_enable_feed_loss).  Without a GPU: the header declares the three names and the library exports each, the NULL-handle calls answer
without touching a device, the header no longer says NOT BUILT for this.  On a GPU (a batch cannot be made without one): every refusal with
nothing changed afterwards, the all-or-nothing check of stream -1, that the call on a strict stream IS tlb_conceal_enable, get / reset /
records on converted streams, and what the three feed setters and the two feed resets do to the state."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_feed_loss_enable", "tlb_tick_enable_feed_loss", "tlb_node_enable_feed_loss"]
ARG = 18


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_the_names(M):
    text = HEADER.read_text()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*feed_loss[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    assert not [n for n in NAMES if "conceal" in n]              # tests/test_conceal_abi.py claims every name with that word, and pins their set
    for n in NAMES:
        assert re.search(r"\bint %s\(tlb_(batch|tick|node) \*\w+, int stream, int hold, int step\);" % n, src), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NAMES) <= exported
    section = text[text.index("CONCEALMENT of lost frames"):text.index("#define TLB_CONCEAL_MAX_HOLD")]
    not_built = section[section.index("NOT BUILT"):]
    assert "adapted" not in not_built and "down feed" not in not_built and "interpolation" in not_built and "feed report" in not_built


def test_null_handles_answer_without_a_gpu(M):
    L = M.load_library()
    assert L.tlb_feed_loss_enable(None, -1, 4, 3) == ARG
    assert L.tlb_tick_enable_feed_loss(None, -1, 4, 3) == ARG
    assert L.tlb_node_enable_feed_loss(None, -1, 4, 3) == ARG


def test_the_python_keyword_defaults_to_todays_call(M):
    import inspect
    for cls in (M.Batch, M.Tick, M.Node):
        p = inspect.signature(cls.enable_conceal).parameters
        assert list(p) == ["self", "hold", "step", "stream", "any_feed"] and p["any_feed"].default is False, cls


# ---- with a batch ----------------------------------------------------------------------------------------------------------------------
def _scfg(M, fs, mode, kbps):
    return M.StreamConfig(samplerate=fs, mode=mode, bitrate=kbps, psy_model=1, pad_len=0)


def _batch(M):
    """five streams: 0, 1 strict feeds (48 kHz stereo 192), 2 an adapted feed (32 kHz into 48 kHz), 3 a down feed (48 kHz into 24 kHz), 4 no feed"""
    b = M.Batch([_scfg(M, 48000, "s", 128)] * 3 + [_scfg(M, 24000, "s", 64), _scfg(M, 48000, "s", 128)])
    fc = M.FeedConfig(48000, 192, 2)
    b.set_feed(0, fc); b.set_feed(1, fc)
    b.set_feed(2, M.FeedConfig(32000, 128, 2), adapt=True)
    b.set_down_feed(3, fc)
    return b, fc


def _code(M, fn, *a, **kw):
    with pytest.raises(M.ToolameError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.gpu
def test_every_refusal_changes_nothing(M):
    b, _ = _batch(M)
    b.enable_conceal(0, 3, any_feed=True)                        # off on a batch that never had it on: nothing happens
    assert _code(M, b.conceal_records) == ARG
    refusals = [dict(stream=4), dict(stream=2, hold=17), dict(stream=3, hold=-1), dict(stream=2, step=0), dict(stream=3, step=22), dict(stream=5),
                dict(stream=-2), dict(stream=-1)]
    for kw in refusals:                                          # no feed at all; hold; step; no such stream; all: stream 4 has no feed
        assert _code(M, b.enable_conceal, any_feed=True, **kw) == ARG, kw
        assert all(b.conceal_cfg(s) is None for s in range(5)), kw
        assert _code(M, b.conceal_records) == ARG, kw            # nothing was allocated either
    b.enable_conceal(4, 3, stream=2, any_feed=True)
    b.enable_conceal(2, 5, stream=3, any_feed=True)
    for kw in refusals:                                          # ... and the same with concealment on for two streams: they keep what they have
        assert _code(M, b.enable_conceal, any_feed=True, **kw) == ARG, kw
        assert [b.conceal_cfg(s) for s in range(5)] == [None, None, (4, 3), (2, 5), None], kw
    for s in (2, 3):                                             # tlb_conceal_enable keeps refusing them, and changes nothing
        assert _code(M, b.enable_conceal, 1, 1, stream=s) == ARG
    assert [b.conceal_cfg(s) for s in range(5)] == [None, None, (4, 3), (2, 5), None]
    rec = b.conceal_records()
    assert rec.shape == (5,) and not rec.view(np.uint8).any()
    b.set_feed(4, M.FeedConfig(48000, 192, 2))                   # every stream has a feed of some kind now: -1 goes through
    b.enable_conceal(16, 21, any_feed=True)
    assert [b.conceal_cfg(s) for s in range(5)] == [(16, 21)] * 5
    b.enable_conceal(0, stream=3, any_feed=True)                 # hold 0: off
    assert b.conceal_cfg(3) is None and b.conceal_cfg(2) == (16, 21)
    b.close()


def _tick(b, kind, frames):
    """one call of one tick of the batch's adapted or down path: frames {stream: bytes} in the streams' first slots, every other slot
    empty -> the tick's PCM [nstreams][2304]"""
    import feeddownlib as FD
    import feedlib as F
    slots = [(frames[i], len(frames[i])) if i in frames else (b"", 0) for i in range(b.nstreams)]
    if kind == "down":
        fr, ln = FD.slots_to_arrays([[[x, (b"", 0)]] for x in slots], b.down_feed_stride)
        return b.down_feed(fr, ln)[0][0]
    fr, ln = F.slots_to_arrays([[x] for x in slots], b.feed_stride)
    return b.feed(fr, ln)[0][0]


@pytest.mark.gpu
def test_enable_feed_on_a_strict_stream_is_enable(M):
    """two strict streams, one enabled through either call: the same parameters, PCM and records over a good frame and two lost ones"""
    import conceallib as K
    import feedlib as F
    frames = K.case_frames(0)
    b = M.Batch([_scfg(M, 48000, "s", 128)] * 2)
    b.set_feed(-1, M.FeedConfig(**F.feed_cfg_of(K.CASES[0])))
    b.enable_conceal(3, 2, stream=0)
    b.enable_conceal(3, 2, stream=1, any_feed=True)
    assert b.conceal_cfg(0) == b.conceal_cfg(1) == (3, 2)
    for fr in (frames[0], None, None):
        slot = (b"", 0) if fr is None else (fr, len(fr))
        a, ln = F.slots_to_arrays([[slot], [slot]], b.feed_stride)
        pcm = b.feed(a, ln)[0]
        rec = b.conceal_records()
        assert np.array_equal(pcm[0, 0], pcm[0, 1]) and pcm[0, 0].any() and rec[0] == rec[1]
    assert (int(rec[1]["concealed"]), int(rec[1]["run"]), int(rec[1]["offset"])) == (2, 2, 4)
    b.close()


@pytest.mark.gpu
def test_get_reset_records_and_what_the_feed_calls_do_to_the_state(M):
    import concealconvlib as V
    adapt, down = V.CASES[0], V.CASES[4]                         # 32 kHz stereo into 48 kHz stereo; 48 kHz stereo into 24 kHz stereo
    fa, fd = V.case_frames(0), V.case_frames(4)
    ca, cd = M.FeedConfig(**V.fcfg_of(adapt)), M.FeedConfig(**V.fcfg_of(down))
    b = M.Batch([_scfg(M, 48000, "s", 128)] * 2 + [_scfg(M, 24000, "s", 64)] * 2)
    for s in (0, 1):
        b.set_feed(s, ca, adapt=True)
    for s in (2, 3):
        b.set_down_feed(s, cd)
    b.enable_conceal(4, 3, any_feed=True)
    assert [b.conceal_cfg(s) for s in range(4)] == [(4, 3)] * 4

    def state(s):
        r = b.conceal_records()[s]
        return tuple(int(r[n]) for n in ("frames", "passed", "concealed", "muted", "run", "offset"))
    # tick 0 with a good frame on every stream (a 1/2 tick wants two: its slot 1 is a lost slot with run 1)
    _tick(b, "adapt", {0: fa[0], 1: fa[0]})
    pcm = _tick(b, "down", {2: fd[0], 3: fd[0]})
    assert pcm[2].any() and np.array_equal(pcm[2], pcm[3])
    assert [state(s) for s in range(4)] == [(1, 1, 0, 0, 0, 0)] * 2 + [(2, 1, 1, 0, 1, 3)] * 2
    b.feed_reset(0)                                              # an adapted stream: G, run and record forgotten, the parameters stay
    b.down_feed_reset(2)                                         # ... and a stream with a down feed
    assert [state(s) for s in range(4)] == [(0,) * 6, (1, 1, 0, 0, 0, 0), (0,) * 6, (2, 1, 1, 0, 1, 3)]
    assert [b.conceal_cfg(s) for s in range(4)] == [(4, 3)] * 4
    b.feed_reset(3); b.down_feed_reset(1)                        # the other family's reset leaves a stream's concealment alone
    assert state(1) == (1, 1, 0, 0, 0, 0) and state(3) == (2, 1, 1, 0, 1, 3)
    b.conceal_reset(1)
    assert state(1) == (0,) * 6 and b.conceal_cfg(1) == (4, 3)
    b.stream_reset(3)                                            # implies tlb_feed_down_reset
    assert state(3) == (0,) * 6 and b.conceal_cfg(3) == (4, 3)
    # each setter switches the stream's concealment off, removal included
    b.set_feed(0, ca, adapt=True)
    assert b.conceal_cfg(0) is None and b.conceal_cfg(1) == (4, 3)
    b.set_feed(1, None)
    assert b.conceal_cfg(1) is None
    b.set_down_feed(2, cd)
    assert b.conceal_cfg(2) is None and b.conceal_cfg(3) == (4, 3)
    b.set_down_feed(3, None)
    assert b.conceal_cfg(3) is None
    b.set_feed(1, M.FeedConfig(48000, 192, 2))                   # a strict feed, concealed, then set again as a strict feed
    b.enable_conceal(2, 2, stream=1, any_feed=True)
    b.set_feed(1, M.FeedConfig(48000, 192, 2))
    assert b.conceal_cfg(1) is None
    # a stream whose concealment is off again decodes a lost slot to silence
    b.set_down_feed(3, cd)
    _tick(b, "down", {3: fd[0]})
    pcm = _tick(b, "down", {})
    assert not pcm[3].any() and not b.conceal_records()[3].tobytes().strip(b"\0")
    b.close()


@pytest.mark.gpu
def test_a_reconfiguration_keeps_the_parameters_and_forgets_the_state(M):
    """tlb_stream_reconfigure with another bitrate on a concealed adapted stream, a concealed down stream and a concealed strict stream:
    every one keeps its hold and step, and G, run and record are forgotten -- the first lost slot behind it is muted, not a repeat of a
    frame from before, and concealment goes on working behind the next good frame.  The records are conceallib.oracle_record's."""
    import concealconvlib as V
    import conceallib as K
    import feedlib as F
    fa, fd, fs = V.case_frames(0), V.case_frames(4), K.case_frames(0)   # 32 kHz stereo into 48 kHz; 48 kHz stereo into 24 kHz; 48 kHz stereo 192 kbps, strict
    b = M.Batch([_scfg(M, 48000, "s", 128), _scfg(M, 24000, "s", 64), _scfg(M, 48000, "s", 128)])
    b.set_feed(0, M.FeedConfig(**V.fcfg_of(V.CASES[0])), adapt=True)
    b.set_down_feed(1, M.FeedConfig(**V.fcfg_of(V.CASES[4])))
    b.set_feed(2, M.FeedConfig(**F.feed_cfg_of(K.CASES[0])))
    b.enable_conceal(4, 3, any_feed=True)

    def ticks(good):
        """four ticks (two when good is 0): a good frame in every stream's first slot of tick `good`, every other slot empty"""
        for t in range(2 if good == 0 else 4):
            _tick(b, "adapt", {0: fa[0], 2: fs[0]} if t == good else {})
            _tick(b, "down", {1: fd[0]} if t == good else {})
        return b.conceal_records().view(K.RECORD_DTYPE)

    def want(lost):
        return K.oracle_record(lost, 4, 3)
    T, G = True, False
    rec = ticks(0)                                               # 3/2: ticks 0 and 1 are wanted; 1/2: both slots of every tick
    assert rec[0] == want([G, T]) and rec[1] == want([G, T, T, T]) and rec[2] == want([G, T])
    assert all(int(rec[s]["concealed"]) > 0 for s in range(3))
    for s, cfg in enumerate((_scfg(M, 48000, "s", 112), _scfg(M, 24000, "s", 56), _scfg(M, 48000, "s", 112))):      # (a frame no longer than the batch's buffers were sized for)
        b.stream_reconfigure(s, cfg)
        assert b.conceal_cfg(s) == (4, 3), s                    # the same answer for all three kinds of feed
        assert not b.conceal_records()[s].tobytes().strip(b"\0"), s
    assert b.feed_adapted(0) and b.down_feed_cfg(1) is not None and b.get_feed(2) is not None
    rec = ticks(1)                                               # from tick 0 again: 3/2 wants ticks 0, 1 and 3
    assert rec[0] == want([T, G, T]) and rec[1] == want([T, T, G, T, T, T, T, T]) and rec[2] == want([T, G, T, T])
    assert [int(rec[s]["muted"]) for s in range(3)] == [1, 2, 1] and all(int(rec[s]["concealed"]) > 0 for s in range(3))
    b.close()
