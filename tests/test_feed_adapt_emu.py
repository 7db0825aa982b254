"""Adapted feeds (csrc/mp2_feed_adapt.h over csrc/mp2_feed.h and csrc/mp2_resample.h) on the lane-loop emulation, without a GPU: the stream
set of feedadaptlib against the numpy oracle -- feedlib's decode of the wanted frames, the channel map, resamplelib's formula -- bit for
bit under every cut; the resample stage alone on full-range input; empty, bad and unwanted slots; a reset mid-run; untouched output; and
hostile bytes and lengths through a program linked with AddressSanitizer + UBSan."""
import shutil

import numpy as np
import pytest

import declib as D
import feedadaptlib as A
import feedlib as F
import resamplelib as R

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
N = A.N
IDS = [("%dk_%s_to_%dk_%s" % (st["feed"][0] // 1000, st["feed"][1], st["enc"][0] // 1000, st["enc"][1])) if st["feed"] else "unfed" for st in A.STREAMS]


def test_the_cases_are_the_ones_asked_for():
    assert [(st["feed"][:3] if st["feed"] else None, st["enc"], st["adapt"]) for st in A.STREAMS] == [
        ((44100, "s", 128), (48000, "s"), True), ((32000, "s", 128), (48000, "m"), True), ((22050, "m", 32), (24000, "s"), True),
        ((16000, "s", 64), (24000, "s"), True), ((48000, "s", 128), (48000, "m"), True), ((48000, "m", 64), (48000, "s"), True),
        ((48000, "s", 192), (48000, "s"), False), (None, (48000, "s"), False)]
    assert A.NTICKS == 14 and A.CUTS == ((14,), (1, 5, 8), (1,) * 14)
    sh = A.shared()
    assert [len(u) for u in sh["used"]] == [13, 10, 13, 10, 14, 14, 14, 0]      # 160/147: tick 12 is unwanted; 3/2: ticks 2, 5, 8, 11
    assert len({len(b) for b in sh["used"][0]}) == 2                             # 44.1 kHz: frames of both lengths


@pytest.fixture(scope="module")
def one_call():
    sh = A.shared()
    e = A.FeedAdaptEmu(A.STREAMS)
    assert e.stride == sh["stride"]
    pcm, rep = e.decode(sh["fr"], sh["ln"])
    e.close()
    return pcm, rep


@pytest.mark.parametrize("s", range(len(A.STREAMS)), ids=IDS)
def test_emulation_equals_the_numpy_oracle(one_call, s):
    """bit for bit; what the call must not write keeps its poison; wanted slots pass, unwanted empty ones read EMPTY"""
    sh = A.shared()
    pcm, rep = one_call
    st = A.STREAMS[s]
    m = A.written(A.STREAMS, A.NTICKS)[:, s]
    assert (pcm[:, s][~m] == A.POISON).all()
    if not st["feed"]:
        assert (rep["status"][:, s] == D.EMPTY).all()
        return
    L, Mm = A.lm_of(st)
    for f in range(A.NTICKS):
        assert int(rep["status"][f, s]) == (0 if A.want(f, L, Mm) else D.EMPTY), (f, hex(int(rep["status"][f, s])))
    got, want = pcm[:, s][m], sh["want"][:, s][m]
    assert np.array_equal(got, want), ("first difference at", np.argwhere(got != want)[:4].tolist(), int(np.abs(got.astype(int) - want.astype(int)).max()))
    assert np.abs(got.astype(int)).max() > 1000                  # audio, not silence


@pytest.mark.parametrize("cuts", A.CUTS[1:], ids=["1+5+8", "14x1"])
def test_the_output_does_not_depend_on_the_cut(one_call, cuts):
    sh = A.shared()
    e = A.FeedAdaptEmu(A.STREAMS)
    pcm, rep = e.run_cuts(sh["fr"], sh["ln"], cuts)
    e.close()
    assert np.array_equal(pcm, one_call[0]) and rep.tobytes() == one_call[1].tobytes()


CHANNELS = [(2, 2), (2, 1), (1, 1), (1, 2)]


@pytest.mark.parametrize("fs,es,nticks", [(44100, 48000, 14), (32000, 48000, 4), (48000, 48000, 2)], ids=["160_147", "3_2", "1_1"])
@pytest.mark.parametrize("fch,sch", CHANNELS, ids=["2to2", "2to1", "1to1", "1to2"])
def test_the_resample_stage_alone_on_full_range_input(fs, es, nticks, fch, sch):
    """full-range random int16 with stretches of L = R = +- full scale and L = -R: pins the channel map ((L + R + 1) >> 1 cannot leave int16)
    and the clamp"""
    L, Mm = A.ratio_of(fs, es)
    total = A.K(nticks - 1, L, Mm) * N
    rng = np.random.default_rng(7 + fch * 2 + sch)
    x = rng.integers(-32768, 32768, (total, fch)).astype(np.int16)
    x[100:400] = 32767
    x[400:700] = -32768
    x[1500:1700] = rng.choice([-32768, 32767], (200, 1))          # full-scale square bursts: the sum overshoots, the clamp acts
    if fch == 2:
        x[700:1000, 0] = 32767; x[700:1000, 1] = -32768           # L = -R - 1: the map gives 0
        x[1000:1200, 0] = -32768; x[1000:1200, 1] = 32767
        x[1200:1300, 1] = -x[1200:1300, 0].clip(-32767, 32767)
    got = A.resample_plane(fs, es, fch, sch, x, nticks)
    want = A.oracle_ticks(x, fs, es, fch, sch, nticks)
    assert np.array_equal(got[:, :N * sch], want[:, :N * sch]) and (got[:, N * sch:] == A.POISON).all()
    if fs != es:
        un = R.oracle_stream(A.channel_map(x, fch, sch), fs, es, N * nticks, unclamped=True)
        assert (((un + 16384) >> 15) > 32767).any() and (((un + 16384) >> 15) < -32768).any()      # the clamp was needed


def _run(streams, lists, cuts=None):
    e = A.FeedAdaptEmu(streams)
    fr, ln = F.slots_to_arrays(lists, e.stride)
    out = e.run_cuts(fr, ln, cuts or (len(lists[0]),))
    e.close()
    return out


def test_an_empty_or_bad_wanted_slot_is_silence_and_keeps_the_schedule():
    """wanted slot 5 of the 44.1 kHz stream left empty / damaged three ways: 1152 zeros of source, its successor decoded as after silence,
    every other frame on the tick it had before"""
    sh = A.shared()
    st = A.STREAMS[0]
    base = sh["lists"][0]
    tick = 5                                                     # (wanted slot 5 is tick 5: the first unwanted tick is 12)
    fr = sh["used"][0][5]
    rng = np.random.default_rng(3)
    variants = dict(empty=(b"", 0, D.EMPTY), random=(rng.integers(0, 256, len(fr), dtype=np.uint8).tobytes(), len(fr), D.BAD_MASK),
                    trunc=(fr[:200], 200, D.OVERRUN), rate=(bytes(bytearray(fr[:2]) + bytearray([fr[2] ^ 0x04]) + bytearray(fr[3:])), len(fr), D.HEADER_MISMATCH))
    lists = []
    for name, (b, n, must) in variants.items():
        sl = list(base); sl[tick] = (b, n); lists.append(sl)
    pcm, rep = _run([st] * len(lists), lists, (6, 8))
    want = A.oracle_pcm([None if k == 5 else f for k, f in enumerate(sh["used"][0])], st)
    for v, (name, (b, n, must)) in enumerate(variants.items()):
        stt = int(rep["status"][tick, v])
        assert stt & must and (name == "empty" or stt & D.BAD_MASK) and not stt & A.UNWANTED, (name, hex(stt))
        assert np.array_equal(pcm[:, v], want), name
        keep = [f for f in range(A.NTICKS) if f != tick]
        assert (rep["status"][keep, v] == [D.EMPTY if f == 12 else 0 for f in keep]).all(), name
    assert not np.array_equal(want, sh["want"][:, 0])


def test_a_non_empty_unwanted_slot_is_reported_and_changes_no_sample(one_call):
    sh = A.shared()
    lists = [list(sl) for sl in sh["lists"]]
    good = sh["used"][0][3]
    lists[0][12] = (good, len(good))                             # 160/147: tick 12
    lists[1][2] = (b"\xff" * 40, 40); lists[1][5] = (sh["used"][1][0], 10 ** 6)      # 3/2: ticks 2 and 5, rubbish and a length beyond the slot
    lists[3][11] = (sh["used"][3][0], len(sh["used"][3][0]))     # the last tick of the run is unwanted: its bytes must not become the history
    pcm, rep = _run(A.STREAMS, lists, (1, 5, 8))
    assert np.array_equal(pcm, one_call[0])
    marked = {(12, 0), (2, 1), (5, 1), (11, 3)}
    for f in range(A.NTICKS):
        for s in range(len(A.STREAMS)):
            want = D.EMPTY | A.UNWANTED if (f, s) in marked else int(one_call[1]["status"][f, s])
            assert int(rep["status"][f, s]) == want, (f, s)
    assert not (A.UNWANTED & D.BAD_MASK)
    # ... and with the unwanted tick as a call's last: the next call's first frame still has the wanted slot before it as its history
    e = A.FeedAdaptEmu([A.STREAMS[1]])
    fr, ln = F.slots_to_arrays([lists[1]], e.stride)
    a, b = e.decode(fr[:3], ln[:3]), e.decode(fr[3:6], ln[3:6])
    e.close()
    assert np.array_equal(np.concatenate([a[0], b[0]])[:, 0], one_call[0][:6, 1])


def test_feed_reset_mid_run_restarts_at_tick_0(one_call):
    sh = A.shared()
    e = A.FeedAdaptEmu(A.STREAMS)
    e.decode(sh["fr"][:5], sh["ln"][:5])
    e.reset(0); e.reset(1)
    pcm, rep = e.decode(sh["fr"][:9], sh["ln"][:9])              # the run from its start again: streams 0 and 1 are at tick 0 ...
    assert np.array_equal(pcm[:, :2], one_call[0][:9, :2]) and rep[:, :2].tobytes() == one_call[1][:9, :2].tobytes()
    e.reset()
    pcm, rep = e.run_cuts(sh["fr"], sh["ln"], (1, 5, 8))
    e.close()
    assert np.array_equal(pcm, one_call[0]) and rep.tobytes() == one_call[1].tobytes()


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------
def hostile_lists():
    """feedlib.hostile_inputs over the first six frames of the 44.1 kHz two-channel and the 32 kHz feed, put on a wanted tick (3) and --
    the damaged bytes -- on an unwanted one (12 / 2) of the same streams' schedules"""
    sh = A.shared()
    streams, lists, marks = [], [], []
    for s, unwanted in ((0, 12), (1, 2)):
        st = A.STREAMS[s]
        for name, slots, must in F.hostile_inputs(sh["used"][s][:F.NFRAMES], A.fcfg_of(st), sh["stride"]):
            bad = slots[F.HOSTILE_SLOT]
            a = list(sh["lists"][s]); a[F.HOSTILE_SLOT] = bad    # tick 3 is wanted for both
            b = list(sh["lists"][s]); b[unwanted] = bad
            streams += [st, st]; lists += [a, b]; marks += [(name, must, F.HOSTILE_SLOT, True), (name, must, unwanted, False)]
    return streams, lists, marks


def noise_calls(ns, stride):
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (A.NTICKS, ns, stride), dtype=np.uint8)
    fr[1] = 0xff
    fr[2, :, :4] = [0xff, 0xfc, 0xf0, 0xff]
    ln = rng.integers(0, stride + 40, (A.NTICKS, ns)).astype(np.int32)
    ln[3] = -5
    ln[12] = 10 ** 9
    return fr, ln


def test_hostile_input_is_flagged_and_contained(one_call):
    sh = A.shared()
    streams, lists, marks = hostile_lists()
    pcm, rep = _run(streams, lists, (1, 5, 8))
    silent = {}
    for v, (name, must, tick, wanted) in enumerate(marks):
        s = 0 if streams[v] is A.STREAMS[0] else 1
        stt = int(rep["status"][tick, v])
        if not wanted:
            assert stt == D.EMPTY | A.UNWANTED, (name, hex(stt))
            assert np.array_equal(pcm[:, v], one_call[0][:, s]), name
            continue
        assert stt & must and stt & D.BAD_MASK and not stt & (D.EMPTY | A.UNWANTED), (name, hex(stt))
        if s not in silent:
            k_bad = A.K(tick, *A.lm_of(streams[v])) - 1           # the wanted slot tick 3 is: 3 for 160/147, 2 for 3/2
            silent[s] = A.oracle_pcm([None if k == k_bad else f for k, f in enumerate(sh["used"][s])], streams[v])
        w = N * A.enc_nch(streams[v])
        assert np.array_equal(pcm[:, v, :w], silent[s][:, :w]) and (pcm[:, v, w:] == A.POISON).all(), name      # zeros of source, the successor's history is silence, whatever the damage was


def test_hostile_input_is_clean_under_asan_ubsan(tmp_path):
    """the same hostile sets, and noise under every kind of length over the whole stream set, through the lane-loop build linked as a
    program with AddressSanitizer + UBSan (tests/emu/mp2_feed_san_main.cpp; its buffers are exactly as long as the data).  Clean,
    and the same reports and PCM as the plain build."""
    exe = A.build_san_driver(tmp_path)
    streams, lists, _ = hostile_lists()
    e = A.FeedAdaptEmu(streams)
    fr, ln = F.slots_to_arrays(lists, e.stride)
    calls = [(fr[:1], ln[:1]), (fr[1:6], ln[1:6]), (fr[6:], ln[6:])]
    (rep, pcm), = A.run_san_driver(exe, tmp_path, streams, [calls])
    want_pcm, want_rep = e.run_cuts(fr, ln, (1, 5, 8))
    e.close()
    assert rep.tobytes() == want_rep.tobytes() and pcm.tobytes() == want_pcm.tobytes()
    e = A.FeedAdaptEmu(A.STREAMS)
    fr, ln = noise_calls(len(A.STREAMS), e.stride)
    (rep, pcm), (rep1, pcm1) = A.run_san_driver(exe, tmp_path, A.STREAMS, [[(fr, ln)], [(fr[f:f + 1], ln[f:f + 1]) for f in range(A.NTICKS)]])
    want_pcm, want_rep = e.decode(fr, ln)
    e.close()
    assert rep.tobytes() == want_rep.tobytes() and pcm.tobytes() == want_pcm.tobytes() == pcm1.tobytes()
    # (tick by tick the status words are the same; the diagnostic CRC of a slot shorter than a header is computed over whatever the parser's
    # buffer held, as on the strict path, and is not compared across cuts)
    assert np.array_equal(rep["status"], rep1["status"])
    m = A.written(A.STREAMS, A.NTICKS)
    assert (pcm[~m] == A.POISON).all()
    for s, st in enumerate(A.STREAMS[:6]):                       # noise decodes to silence: every adapted stream's output is zeros
        assert not pcm[:, s][m[:, s]].any()
        L, Mm = A.lm_of(st)
        for f in range(A.NTICKS):
            stt = int(rep["status"][f, s])
            if not A.want(f, L, Mm):
                assert stt == (D.EMPTY | A.UNWANTED if ln[f, s] > 0 else D.EMPTY)
            else:
                assert stt & D.BAD_MASK if ln[f, s] > 0 else stt == D.EMPTY
