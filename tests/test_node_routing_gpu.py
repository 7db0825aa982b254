"""How the node (csrc/tlb_node.cpp) routes a caller's stream id to a shard and a shard-local id, and what it answers a caller's mistake:
pinned through the raw C-ABI of the product library, on the smallest shapes at which the routing can go wrong.  5 streams over
devices = (0, 0) are shard blocks [0, 2) and [2, 5); ngroups = 2 cuts those into tick groups of 1 + 1 and 1 + 2 streams, so streams 1, 2
and 3 each sit at an edge of a block or of a group.  48 kHz 128 kbps psy 1, stream 3 mono and the others stereo.

(a) every per-stream answer of the node equals, byte for byte, the answer of ONE tlb_tick over the same five streams;
(b) the empty answers (NULL / 0 / *len = 0 / the argument error) of every early return;
(c) the order in which the two remembered setters (tlb_node_set_source, tlb_node_set_feed) check their arguments.

One case differs from the five streams above: tlb_node_set_feed(-1, cfg) gives every stream ONE channel count, so the feed run of (a)
makes stream 3 stereo as well (with the mono stream the call is TLB_ERR_MODE on node and twin alike, which (c) asserts)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, SAMPLERATE, MODE, HIP, ARG = 0, 1, 2, 17, 18
NS, OUTSIDE = 5, (-1, 5)
NOW_S = 1712345678
EGRESS = {"frames": 0, "af": 1}


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def _cfgs(M, mono=(3,)):
    return [M.StreamConfig(samplerate=48000, mode="m" if s in mono else "s", bitrate=128, psy_model=1) for s in range(NS)]


def _tick_config(M, egress, ngroups, with_xpad=0):
    return M.toolame._CTickConfig(EGRESS[egress], ngroups, with_xpad, b"rt", 2, NOW_S, 0, 0, 37, 0, 207, 0, 0, 0)


def _node(M, L, cfgs, egress="af", plane=0, with_xpad=0):
    nc = M.toolame._CNodeConfig()
    nc.plane = plane
    nc.tick = _tick_config(M, egress, 2, with_xpad)
    err = C.c_int(-1)
    nd = L.tlb_node_create(2, (C.c_int * 2)(0, 0), NS, M.toolame._config_array(cfgs), C.byref(nc), C.byref(err))
    assert nd and err.value == OK, err.value
    return nd


def _twin(M, L, cfgs, egress):
    tc = _tick_config(M, egress, 1)
    err = C.c_int(-1)
    t = L.tlb_tick_create(0, NS, M.toolame._config_array(cfgs), C.byref(tc), C.byref(err))
    assert t and err.value == OK, err.value
    return t


def _bytes(p, n):
    return C.string_at(p, n) if p else None


def _with_len(fn, *args):
    """(the bytes or None, *len) of an accessor that reports a length; len is preset to 77"""
    n = C.c_int(77)
    p = fn(*args, C.byref(n))
    return (_bytes(p, n.value), n.value)


def _node_answers(L, nd, s):
    units = L.tlb_node_units(nd, s)
    return (units, _bytes(L.tlb_node_peaks(nd, s), 4), L.tlb_node_silence_ms(nd, s), _with_len(L.tlb_node_frame, nd, s),
            [_with_len(L.tlb_node_packet, nd, s, u) for u in range(units)])


def _twin_answers(L, t, s):
    units = L.tlb_tick_units(t, s)
    peaks, silence = L.tlb_tick_peaks(t), L.tlb_tick_silence_ms(t)
    return (units, _bytes(peaks + 4 * s, 4), C.c_uint32.from_address(silence + 4 * s).value, _with_len(L.tlb_tick_frame, t, s),
            [_with_len(L.tlb_tick_packet, t, s, u) for u in range(units)])


@pytest.mark.parametrize("egress,setting", [("af", "gain"), ("af", "source"), ("af", "feed"), ("frames", "gain")])
def test_every_stream_of_the_node_answers_what_one_tick_object_answers(M, egress, setting):
    L = M.load_library()
    cfgs = _cfgs(M, mono=() if setting == "feed" else (3,))
    nd, t = _node(M, L, cfgs, egress), _twin(M, L, cfgs, egress)
    try:
        if setting == "gain":
            assert L.tlb_node_set_gain_db(nd, 2, -6.0) == OK and L.tlb_tick_set_gain_db(t, 2, -6.0) == OK
        elif setting == "source":
            assert L.tlb_node_set_source(nd, 4, 44100) == OK and L.tlb_tick_set_source(t, 4, 44100) == OK
        else:
            fc = M.toolame._CFeedConfig(48000, 192, 2)
            assert L.tlb_node_set_feed(nd, -1, C.byref(fc)) == OK and L.tlb_tick_set_feed(t, -1, C.byref(fc)) == OK
            assert L.tlb_node_set_feed(nd, 1, None) == OK and L.tlb_tick_set_feed(t, 1, None) == OK
            stride = L.tlb_tick_feed_stride(t)
            assert stride > 0 and [L.tlb_node_feed_stride(nd, s) for s in range(NS)] == [stride] * NS
            assert all(L.tlb_node_feed(nd, s) and L.tlb_node_feed_len(nd, s) for s in range(NS))
            # a different programme per stream as 576-byte Layer II frames: a slot routed to the wrong local id changes that stream's packets
            enc = M.Batch([M.StreamConfig(mode="s", bitrate=192, psy_model=1)] * NS)
            src = np.random.default_rng(32).integers(-9000, 9000, size=(4, NS, 2, 1152), dtype=np.int16)
            feeds = [a + b for a, b in zip(enc.encode(src)[0], enc.flush())]
            enc.close()
            assert all(len(x) == 4 * 576 for x in feeds) and stride >= 576
        pcm = np.random.default_rng(31).integers(-9000, 9000, size=(3, NS, 2304), dtype=np.int16)
        some = 0
        for f in range(3):
            if setting == "source":
                need = L.tlb_tick_need(t, 4)
                assert 0 < need < 1152 and L.tlb_node_need(nd, 4) == need, (f, need)
                assert [L.tlb_node_need(nd, s) for s in range(4)] == [L.tlb_tick_need(t, s) for s in range(4)] == [1152] * 4
            base = L.tlb_tick_pcm(t)
            for s in range(NS):
                p = L.tlb_node_pcm(nd, s)
                assert p and base
                C.memmove(p, pcm[f, s].ctypes.data, 4608)
                C.memmove(base + 4608 * s, pcm[f, s].ctypes.data, 4608)
            for s in range(NS) if setting == "feed" else ():
                fr, base, lens = feeds[s][576 * f:576 * (f + 1)], L.tlb_tick_feed(t), L.tlb_tick_feed_len(t)
                C.memmove(L.tlb_node_feed(nd, s), fr, 576)
                C.memmove(base + stride * s, fr, 576)
                C.c_int32.from_address(L.tlb_node_feed_len(nd, s)).value = C.c_int32.from_address(lens + 4 * s).value = 576 * (s != 1)
            assert L.tlb_node_run(nd) == OK and L.tlb_tick_run(t) == OK
            for s in range(NS):
                got, want = _node_answers(L, nd, s), _twin_answers(L, t, s)
                assert got == want, (f, s)
                some += sum(n for _, n in got[4]) + got[3][1] * (egress == "frames")
            if setting == "source":
                assert L.tlb_node_need(nd, 4) == L.tlb_tick_need(t, 4)
        assert some > 0                                              # (the comparison was of packets / frames, not of empty slots)
    finally:
        L.tlb_node_destroy(nd)
        L.tlb_tick_destroy(t)


@pytest.fixture(scope="module")
def tick_node(M):
    L = M.load_library()
    nd = _node(M, L, _cfgs(M))
    yield nd
    L.tlb_node_destroy(nd)


@pytest.fixture(scope="module")
def batch_node(M):
    L = M.load_library()
    nb = _node(M, L, _cfgs(M), plane=1)
    yield nb
    L.tlb_node_destroy(nb)


POINTERS = ("tlb_node_pcm", "tlb_node_xpad", "tlb_node_xpad_len", "tlb_node_peaks", "tlb_node_monitor", "tlb_node_compare", "tlb_node_feed",
            "tlb_node_feed_len", "tlb_node_feed_report", "tlb_node_valid")
COUNTS = ("tlb_node_units", "tlb_node_silence_ms", "tlb_node_underrun_ms", "tlb_node_underruns", "tlb_node_feed_stride")


def _lens(L, nd, s):
    """[(pointer, *len)] of the four accessors that report a length"""
    out = []
    for fn, args in ((L.tlb_node_frame, ()), (L.tlb_node_packet, (0,)), (L.tlb_node_message, (0,)), (L.tlb_node_fragment, (0, 0))):
        n = C.c_int(77)
        out.append((fn(nd, s, *args, C.byref(n)), n.value))
    return out


def test_a_stream_outside_the_node_and_no_node_answer_nothing(M, tick_node):
    L, nd = M.load_library(), tick_node
    for s in OUTSIDE:
        assert [getattr(L, f)(nd, s) for f in POINTERS] == [None] * len(POINTERS), s
        assert [getattr(L, f)(nd, s) for f in COUNTS] == [0] * len(COUNTS) and L.tlb_node_fragments(nd, s, 0) == 0, s
        assert _lens(L, nd, s) == [(None, 0)] * 4, s
        assert L.tlb_node_need(nd, s) == -ARG and L.tlb_node_shard_of(nd, s) == -1
        assert L.tlb_node_stream_reset(nd, s) == ARG
        assert L.tlb_node_stream_reconfigure(nd, s, M.toolame._config_array(_cfgs(M)[:1])) == ARG
        out = C.create_string_buffer(4096)
        assert L.tlb_node_stream_finish(nd, s, out, 4096) == -ARG
    assert [getattr(L, f)(None, 0) for f in POINTERS] == [None] * len(POINTERS)
    assert [getattr(L, f)(None, 0) for f in COUNTS] == [0] * len(COUNTS) and L.tlb_node_fragments(None, 0, 0) == 0
    assert L.tlb_node_monitor_pcm(None, None) is None
    assert L.tlb_node_need(None, 0) == -ARG and L.tlb_node_shard_of(None, 0) == -1
    assert [L.tlb_node_shard_of(nd, s) for s in range(NS)] == [0, 0, 1, 1, 1]


def test_each_plane_refuses_the_other_planes_calls(M, tick_node, batch_node):
    L, nd, nb = M.load_library(), tick_node, batch_node
    for s in range(NS):
        assert [getattr(L, f)(nb, s) for f in POINTERS] == [None] * len(POINTERS), s
        assert [getattr(L, f)(nb, s) for f in COUNTS] == [0] * len(COUNTS) and L.tlb_node_fragments(nb, s, 0) == 0, s
        assert [p for p, _ in _lens(L, nb, s)] == [None] * 4, s
        assert L.tlb_node_need(nb, s) == -ARG
    listened = C.c_int(3)
    assert L.tlb_node_monitor_pcm(nb, C.byref(listened)) is None and listened.value == -1
    assert L.tlb_node_submit(nb) == ARG and L.tlb_node_wait(nb) == ARG and L.tlb_node_finish(nb) == ARG
    assert L.tlb_node_encode_device(nd, None, 1, None, None, None, None) == ARG
    assert L.tlb_node_flush_device(nd, None, None) == ARG and L.tlb_node_sync(nd) == ARG


def test_an_option_never_enabled_answers_nothing(M, tick_node):
    L, nd = M.load_library(), tick_node
    for s in range(NS):
        for f in ("tlb_node_valid", "tlb_node_monitor", "tlb_node_compare", "tlb_node_feed", "tlb_node_feed_len", "tlb_node_feed_report"):
            assert getattr(L, f)(nd, s) is None, (f, s)
        assert (L.tlb_node_underrun_ms(nd, s), L.tlb_node_underruns(nd, s), L.tlb_node_feed_stride(nd, s)) == (0, 0, 0), s
    listened = C.c_int(3)
    assert L.tlb_node_monitor_pcm(nd, C.byref(listened)) is None and listened.value == -1


def test_no_input_set_is_free_while_two_ticks_are_in_flight_and_no_setter_runs(M):
    L = M.load_library()
    nd = _node(M, L, _cfgs(M), with_xpad=1)
    inputs = lambda s: (L.tlb_node_pcm(nd, s), L.tlb_node_xpad(nd, s), L.tlb_node_xpad_len(nd, s))
    fc = M.toolame._CFeedConfig(48000, 192, 2)

    def fill():
        for s in range(NS):
            pcm, xpad, xlen = inputs(s)
            assert pcm and xpad and xlen, s
            C.memset(pcm, 0, 4608)
            C.memset(xlen, 0, 4)
    try:
        fill()
        assert L.tlb_node_submit(nd) == OK
        # (c) a tick in flight: neither remembered setter runs
        assert L.tlb_node_set_source(nd, 4, 44100) == ARG and L.tlb_node_set_feed(nd, 0, C.byref(fc)) == ARG and L.tlb_node_set_feed(nd, 0, None) == ARG
        fill()
        assert L.tlb_node_submit(nd) == OK
        assert all(inputs(s) == (None, None, None) for s in range(NS))
        assert L.tlb_node_submit(nd) == ARG
        assert L.tlb_node_wait(nd) == OK
        assert all(all(inputs(s)) for s in range(NS))
        assert L.tlb_node_wait(nd) == OK
        assert L.tlb_node_need(nd, 4) == 1152 and L.tlb_node_feed_stride(nd, 0) == 0
    finally:
        L.tlb_node_destroy(nd)


def test_the_remembered_setters_check_in_their_order_and_change_nothing_when_they_refuse(M, tick_node):
    L, nd = M.load_library(), tick_node
    need = [L.tlb_node_need(nd, s) for s in range(NS)]
    assert need == [1152] * NS
    assert L.tlb_node_set_source(nd, 0, 12345) == SAMPLERATE and L.tlb_node_set_source(nd, -1, 12345) == SAMPLERATE
    assert [L.tlb_node_need(nd, s) for s in range(NS)] == need
    for s in OUTSIDE[1:] + (-2,):
        assert L.tlb_node_set_source(nd, s, 44100) == ARG and L.tlb_node_set_feed(nd, s, None) == ARG
    assert L.tlb_node_set_source(nd, 0, -1) == ARG and L.tlb_node_set_source(None, 0, 44100) == ARG and L.tlb_node_set_feed(None, 0, None) == ARG
    stereo, mono = M.toolame._CFeedConfig(48000, 192, 2), M.toolame._CFeedConfig(48000, 96, 1)
    assert L.tlb_node_set_feed(nd, 3, C.byref(stereo)) == MODE and L.tlb_node_set_feed(nd, 2, C.byref(mono)) == MODE
    assert L.tlb_node_set_feed(nd, -1, C.byref(stereo)) == MODE and L.tlb_node_set_feed(nd, -1, C.byref(mono)) == MODE
    assert L.tlb_node_set_feed(nd, 0, C.byref(M.toolame._CFeedConfig(24000, 160, 2))) == SAMPLERATE
    assert L.tlb_node_set_feed(nd, -1, None) == OK and L.tlb_node_set_source(nd, -1, 0) == OK      # (never on, cleared: nothing happens)
    assert [L.tlb_node_feed_stride(nd, s) for s in range(NS)] == [0] * NS and [L.tlb_node_need(nd, s) for s in range(NS)] == need


def test_a_feed_or_a_source_is_refused_while_short_reads_are_enabled(M):
    L = M.load_library()
    nd = _node(M, L, _cfgs(M))
    try:
        assert L.tlb_node_enable_short_reads(nd) == OK and all(L.tlb_node_valid(nd, s) for s in range(NS))
        assert L.tlb_node_set_feed(nd, 0, C.byref(M.toolame._CFeedConfig(48000, 192, 2))) == ARG
        assert L.tlb_node_set_feed(nd, 3, C.byref(M.toolame._CFeedConfig(48000, 192, 2))) == MODE       # (the stream's fit is checked first)
        assert L.tlb_node_set_source(nd, 4, 44100) == ARG and L.tlb_node_set_source(nd, 4, 12345) == SAMPLERATE
        assert L.tlb_node_set_source(nd, 4, 48000) == OK and L.tlb_node_set_feed(nd, -1, None) == OK     # no real source, no feed: allowed
        assert [L.tlb_node_feed_stride(nd, s) for s in range(NS)] == [0] * NS and [L.tlb_node_need(nd, s) for s in range(NS)] == [1152] * NS
        assert all(L.tlb_node_feed(nd, s) is None and L.tlb_node_valid(nd, s) for s in range(NS))
    finally:
        L.tlb_node_destroy(nd)
