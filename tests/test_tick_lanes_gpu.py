"""The two feed lanes of a tick object (csrc/tlb_tick.cpp: Layer II feeds and down feeds go through one set body, one refresh and one loop in
submit, egress and wait): what only one of the two families had a test for, asked of both.  Streams of 24 kHz in two groups, three ticks,
`frames` egress; the frame material is what tests/feedlib.py and tests/feeddownlib.py build."""
import numpy as np
import pytest

import feeddownlib as A
import feedlib as F

pytestmark = pytest.mark.gpu
NTICKS = 3


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


class FeedLane:
    """strict feeds: stream 0 is mono and gets the narrow feed, stream 1 is stereo and gets the wide one"""
    cases = [(24000, "m", 32, 0), (24000, "s", 64, 3)]

    def __init__(self):
        self.modes = [c[1] for c in self.cases]
        self.fcfgs = [F.feed_cfg_of(c) for c in self.cases]
        self.frames = [F.oracle_frames(c, F.case_pcm(i, c, NTICKS)) for i, c in enumerate(self.cases)]

    def set(self, t, s, cfg):
        t.set_feed(s, cfg)

    def views(self, t):
        return t.feed, t.feed_len, t.feed_report, t.feed_stride

    def fill(self, t, f, src_of):
        fr, ln, _, _ = self.views(t)
        assert not ln.any()
        for s in range(t.nstreams):
            b = self.frames[src_of(s)][f]
            fr[s, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            ln[s] = len(b)


class DownFeedLane:
    """48 kHz down feeds (two frames every tick): a 64 kbps mono one for the mono stream 0, a 192 kbps stereo one for the stereo stream 1"""
    streams = [A.STREAMS[5], A.STREAMS[0]]

    def __init__(self):
        self.modes = [st["mode"] for st in self.streams]
        self.fcfgs = [A.fcfg_of(st) for st in self.streams]
        self.lists, _ = A.slots_on_schedule(self.streams, NTICKS)

    def set(self, t, s, cfg):
        t.set_down_feed(s, cfg)

    def views(self, t):
        return t.down_feed, t.down_feed_len, t.down_feed_report, t.down_feed_stride

    def fill(self, t, f, src_of):
        fr, ln, _, _ = self.views(t)
        assert not ln.any()
        for s in range(t.nstreams):
            assert t.down_feed_want(s) == 2
            for j, (b, n) in enumerate(self.lists[src_of(s)][f]):
                fr[s, j, :len(b)] = np.frombuffer(b, dtype=np.uint8)
                ln[s, j] = n


_lanes = {}


def lane_of(name):
    if name not in _lanes:
        _lanes[name] = dict(feed=FeedLane, down_feed=DownFeedLane)[name]()
    return _lanes[name]


def ticks_equal(lane, a, b, src_of):
    """three fed ticks on both objects: frames and reports equal byte for byte, every report good, a frame out from the second tick on"""
    for f in range(NTICKS):
        for x in (a, b):
            x.pcm[:] = 0
            lane.fill(x, f, src_of)
            x.run()
        ra, rb = lane.views(a)[2], lane.views(b)[2]
        assert ra.tobytes() == rb.tobytes() and not ra["status"].any(), f
        for s in range(a.nstreams):
            assert a.frame(s) == b.frame(s) and (f == 0 or len(a.frame(s)) > 0), (f, s)


@pytest.mark.parametrize("name", ["feed", "down_feed"])
def test_a_wider_feed_replaces_the_frame_buffers_and_the_object_equals_its_twin(M, name):
    """Object A sets the narrow configuration on stream 0, then the wide one on stream 1: the lane's slot width grows and its frame buffers are
    replaced.  Twin B sets the wide one first (its buffers are made once; the width only grows).  The accessors are fetched again after every
    set, as their contract says, and show the new width."""
    lane = lane_of(name)
    scfgs = [M.StreamConfig(samplerate=24000, mode=m, bitrate=64, psy_model=1) for m in lane.modes]
    narrow, wide = (M.FeedConfig(**c) for c in lane.fcfgs)
    nb, wb = (F.slot_bytes(c) for c in lane.fcfgs)
    assert nb < wb
    a, b = M.Tick(scfgs, egress="frames", ngroups=2), M.Tick(scfgs, egress="frames", ngroups=2)
    assert lane.views(a) == (None, None, None, 0)
    lane.set(a, 0, narrow)
    fr, ln, rep, stride = lane.views(a)
    assert stride == nb and fr.shape[0] == 2 and fr.shape[-1] == nb and fr.size == ln.size * nb and rep.size == ln.size
    lane.set(a, 1, wide)
    lane.set(b, 1, wide); lane.set(b, 0, narrow)
    for x in (a, b):
        fr, ln, rep, stride = lane.views(x)                          # fetched again: the wide buffers
        assert stride == wb and fr.shape[-1] == wb and fr.size == ln.size * wb and not ln.any()
    ticks_equal(lane, a, b, lambda s: s)
    a.close(); b.close()


def test_a_refused_set_down_feed_leaves_no_down_feed_and_the_accepted_one_equals_the_twin(M):
    """tlb_tick_set_down_feed is all or nothing, as tlb_tick_set_feed is (tests/test_feed_gpu.py): the fault-injection build refuses the nth
    allocation of the library's memory owner for nth = 1, 2, ... until the call is accepted.  Every refused attempt answers TLB_ERR_HIP and
    leaves no stream with a down feed and the object healthy; the object then produces the frames of a twin that set its down feeds with
    nothing armed."""
    FI = M.load_fault_library()
    lane = lane_of("down_feed")
    scfgs = [M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1)] * 4
    fc = M.FeedConfig(**lane.fcfgs[1])
    t, twin = M.Tick(scfgs, egress="frames", ngroups=2, lib=FI), M.Tick(scfgs, egress="frames", ngroups=2, lib=FI)
    twin.set_down_feed(-1, fc)
    refused = 0
    try:
        for nth in range(1, 65):
            assert FI.tlb_debug_alloc_fail_next(nth) == 0
            try:
                t.set_down_feed(-1, fc)
                break
            except M.ToolameError as e:
                assert e.code == 17, (nth, e.code)
            assert t.down_feed is None and t.down_feed_len is None and t.down_feed_report is None and t.down_feed_stride == 0 and t.status() == 0, nth
            refused += 1
        else:
            pytest.fail("not accepted")
    finally:
        FI.tlb_debug_alloc_fail_next(0)
    assert refused >= 4                                              # lengths and reports, the frame buffers, each group's batch
    ticks_equal(lane, t, twin, lambda s: 1)
    t.close(); twin.close()
