"""Down feeds (csrc/mp2_feed_down.h over csrc/mp2_feed.h and csrc/mp2_decimate.h) on the lane-loop emulation, without a GPU: the stream set
of feeddownlib against the numpy oracle -- feedlib's decode of the wanted frames, the channel map, decimatelib's formula -- bit for bit
under every cut; the decimate stage alone on full-range input; empty and bad frames in either slot; slot 1 on a one-frame tick; a reset
mid-run; untouched output; and hostile bytes and lengths through a program linked with AddressSanitizer + UBSan."""
import shutil

import numpy as np
import pytest

import decimatelib as DC
import declib as D
import feeddownlib as A

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
N = A.N
IDS = [("%dk_%s_to_24k_%s" % (st["feed"][0] // 1000, st["feed"][1], st["mode"])) if st["feed"] else "unfed" for st in A.STREAMS]


def test_the_cases_are_the_ones_asked_for():
    assert [(st["feed"][:3] if st["feed"] else None, st["mode"]) for st in A.STREAMS] == [
        ((48000, "s", 192), "s"), ((48000, "s", 128), "m"), ((44100, "s", 128), "s"), ((32000, "m", 64), "s"), ((32000, "s", 128), "m"),
        ((48000, "m", 64), "m"), (None, "s")]
    assert A.NTICKS == 8 and A.CUTS == ((8,), (1, 3, 4), (1,) * 8)
    sh = A.shared()
    assert [len(u) for u in sh["used"]] == [16, 16, 15, 11, 11, 16, 0]           # 80/147: tick 6 wants one frame; 3/4: 2, 1, 1, ...
    assert len({len(b) for b in sh["used"][2]}) == 2                             # 44.1 kHz: frames of both lengths
    assert sh["stride"] == 576


@pytest.fixture(scope="module")
def one_call():
    sh = A.shared()
    e = A.FeedDownEmu(A.STREAMS)
    assert e.stride == sh["stride"]
    pcm, rep = e.decode(sh["fr"], sh["ln"])
    assert [e.pos(s) for s in range(len(A.STREAMS))] == [0, 0, 8, 2, 2, 0, 0]
    e.close()
    return pcm, rep


@pytest.mark.parametrize("s", range(len(A.STREAMS)), ids=IDS)
def test_emulation_equals_the_numpy_oracle(one_call, s):
    """bit for bit; what the call must not write keeps its poison; wanted slots pass, slot 1 of a one-frame tick reads EMPTY"""
    sh = A.shared()
    pcm, rep = one_call
    st = A.STREAMS[s]
    m = A.written(A.STREAMS, A.NTICKS)[:, s]
    assert (pcm[:, s][~m] == A.POISON).all()
    wanted, other = A.expected_status(A.STREAMS, sh["ln"])
    assert (rep["status"][:, s][wanted[:, s]] == 0).all() and np.array_equal(rep["status"][:, s][~wanted[:, s]], other[:, s][~wanted[:, s]])
    if not st["feed"]:
        assert not wanted[:, s].any()
        return
    assert not (other[:, s] & A.UNWANTED).any()
    got, want = pcm[:, s][m], sh["want"][:, s][m]
    assert np.array_equal(got, want), ("first difference at", np.argwhere(got != want)[:4].tolist(), int(np.abs(got.astype(int) - want.astype(int)).max()))
    assert np.abs(got.astype(int)).max() > 1000                  # audio, not silence


@pytest.mark.parametrize("cuts", A.CUTS[1:], ids=["1+3+4", "8x1"])
def test_the_output_does_not_depend_on_the_cut(one_call, cuts):
    sh = A.shared()
    e = A.FeedDownEmu(A.STREAMS)
    pcm, rep = e.run_cuts(sh["fr"], sh["ln"], cuts)
    e.close()
    assert np.array_equal(pcm, one_call[0]) and rep.tobytes() == one_call[1].tobytes()


CHANNELS = [(2, 2), (2, 1), (1, 1), (1, 2)]


@pytest.mark.parametrize("fs,cuts", [(48000, (1, 2)), (32000, (2, 1, 4)), (44100, (79, 3))], ids=["1_2", "3_4", "80_147"])
@pytest.mark.parametrize("fch,sch", CHANNELS, ids=["2to2", "2to1", "1to1", "1to2"])
def test_the_decimate_stage_alone_on_full_range_input(fs, cuts, fch, sch):
    """full-range random int16 with stretches of +- full scale, of L = -R - 1 and decimatelib's adversarial row: pins the channel map
    ((L + R + 1) >> 1 cannot leave int16), the clamp and the split of the sum into 32-bit quarters added in 64 bits.  80/147 runs over 82
    ticks cut (79, 3): the position wraps at 80 between the calls."""
    L, Mm = A.RATIOS[fs]
    nticks = sum(cuts)
    total = A.K(nticks - 1, L, Mm) * N
    rng = np.random.default_rng(7 + fch * 2 + sch)
    x = rng.integers(-32768, 32768, (total, fch)).astype(np.int16)
    adv, n_adv, _ = DC.adversarial(fs, A.ES)                      # drives output n_adv of a one-channel stream to the largest quarter sums
    x[:len(adv)] = adv
    a = len(adv) + 64
    x[a:a + 300] = 32767
    x[a + 300:a + 600] = -32768
    x[a + 1400:a + 1600] = rng.choice([-32768, 32767], (200, 1))  # full-scale square bursts: the sum overshoots, the clamp acts
    if fch == 2:
        x[a + 600:a + 900, 0] = 32767; x[a + 600:a + 900, 1] = -32768      # L = -R - 1: the map gives 0
        x[a + 900:a + 1100, 0] = -32768; x[a + 900:a + 1100, 1] = 32767
    got = A.decimate_plane(fs, fch, sch, x, cuts)
    xm = A.channel_map(x, fch, sch)
    # the oracle over the whole run is a Python loop per output: the first two ticks, the ticks around every cut and the last one
    ticks = sorted({0, 1, nticks - 1} | {t for c in np.cumsum(cuts)[:-1] for t in (c - 1, c, c + 1) if t < nticks})
    for t in ticks:
        y = DC.oracle_stream(xm, fs, A.ES, N, n0=N * t)
        if fch == 1 and sch == 2:
            y = np.repeat(y, 2, axis=1)
        assert np.array_equal(got[t, :N * sch], y.astype(np.int16).reshape(-1)), t
    assert (got[:, N * sch:] == A.POISON).all()
    un = DC.oracle_stream(xm, fs, A.ES, 2 * N, unclamped=True)
    assert (((un + 16384) >> 15) > 32767).any() and (((un + 16384) >> 15) < -32768).any()      # the clamp was needed
    if fch == 1 and fs == 32000:                                  # sum |H[p]| = 67 496 for 3/4: the exact sum is outside 32 bits (1/2 and 80/147 stay just
        assert abs(int(un[n_adv, 0])) >= 2 ** 31                  # inside, as tests/test_decimate_emu.py notes): the 64-bit sum of the quarters was needed


def _run(streams, lists, cuts=None):
    e = A.FeedDownEmu(streams)
    fr, ln = A.slots_to_arrays(lists, e.stride)
    out = e.run_cuts(fr, ln, cuts or (len(lists[0]),))
    e.close()
    return out


def _damaged(fr, rng):
    """an empty, a random, a truncated and a wrong-rate frame in place of `fr` -> {name: (bytes, length, a flag that must be set)}"""
    return dict(empty=(b"", 0, D.EMPTY), random=(rng.integers(0, 256, len(fr), dtype=np.uint8).tobytes(), len(fr), D.BAD_MASK),
                trunc=(fr[:200], 200, D.OVERRUN), rate=(bytes(bytearray(fr[:2]) + bytearray([fr[2] ^ 0x04]) + bytearray(fr[3:])), len(fr), D.HEADER_MISMATCH))


@pytest.mark.parametrize("slot", [0, 1])
def test_an_empty_or_bad_frame_is_silence_and_keeps_the_schedule(slot):
    """the 44.1 kHz stream's tick 3 (a two-frame tick) with slot 0 or slot 1 left empty or damaged three ways: 1152 zeros of source, the
    successor decoded as after silence, every other frame on the tick it had"""
    sh = A.shared()
    s, tick = 2, 3
    st = A.STREAMS[s]
    L, Mm = A.lm_of(st)
    assert A.want(tick, L, Mm) == 2
    k_bad = A.K(tick - 1, L, Mm) + slot                           # the wanted frame that slot holds
    variants = _damaged(sh["used"][s][k_bad], np.random.default_rng(3))
    lists = []
    for name, (b, n, must) in variants.items():
        sl = [list(p) for p in sh["lists"][s]]
        sl[tick][slot] = (b, n)
        lists.append(sl)
    pcm, rep = _run([st] * len(lists), lists, (4, 4) if slot else (3, 5))        # the damaged slot is a call's last wanted one, or its first
    want = A.oracle_pcm([None if k == k_bad else f for k, f in enumerate(sh["used"][s])], st)
    wanted, _ = A.expected_status([st], sh["ln"][:, s:s + 1])
    for v, (name, (b, n, must)) in enumerate(variants.items()):
        stt = int(rep["status"][tick, v, slot])
        assert stt & must and (name == "empty" or stt & D.BAD_MASK) and not stt & A.UNWANTED, (name, hex(stt))
        assert np.array_equal(pcm[:, v], want), name
        keep = wanted[:, 0].copy(); keep[tick, slot] = False
        assert (rep["status"][:, v][keep] == 0).all() and (rep["status"][:, v][~wanted[:, 0]] == D.EMPTY).all(), name
    assert not np.array_equal(want, sh["want"][:, s])


def test_slot_1_of_a_one_frame_tick_is_reported_and_changes_no_sample(one_call):
    sh = A.shared()
    lists = [[list(p) for p in sl] for sl in sh["lists"]]
    good = sh["used"][2][3]
    lists[2][6][1] = (good, len(good))                            # 80/147: tick 6 wants one frame
    lists[3][1][1] = (b"\xff" * 40, 40); lists[3][2][1] = (sh["used"][3][0], 10 ** 6)      # 3/4: ticks 1 and 2, rubbish and a length beyond the slot
    lists[4][7][1] = (sh["used"][4][0], len(sh["used"][4][0]))    # the run's last tick wants one: slot 1's bytes must not become the history
    pcm, rep = _run(A.STREAMS, lists, (1, 3, 4))
    assert np.array_equal(pcm, one_call[0])
    marked = {(6, 2), (1, 3), (2, 3), (7, 4)}
    for f in range(A.NTICKS):
        for s in range(len(A.STREAMS)):
            assert int(rep["status"][f, s, 0]) == int(one_call[1]["status"][f, s, 0])
            want = D.EMPTY | A.UNWANTED if (f, s) in marked else int(one_call[1]["status"][f, s, 1])
            assert int(rep["status"][f, s, 1]) == want, (f, s)
    assert not (A.UNWANTED & D.BAD_MASK)
    # ... and with that tick as a call's last: the next call's first frame still has the wanted slot 0 before it as its history
    e = A.FeedDownEmu([A.STREAMS[3]])
    fr, ln = A.slots_to_arrays([lists[3]], e.stride)
    a, b = e.decode(fr[:3], ln[:3]), e.decode(fr[3:6], ln[3:6])
    e.close()
    assert np.array_equal(np.concatenate([a[0], b[0]])[:, 0], one_call[0][:6, 3])


def test_a_reset_mid_run_restarts_at_tick_0(one_call):
    sh = A.shared()
    e = A.FeedDownEmu(A.STREAMS)
    e.decode(sh["fr"][:5], sh["ln"][:5])
    e.reset(2); e.reset(3)
    pcm, rep = e.decode(sh["fr"][:7], sh["ln"][:7])               # the run from its start again: streams 2 and 3 are at tick 0 ...
    assert np.array_equal(pcm[:, 2:4], one_call[0][:7, 2:4]) and rep[:, 2:4].tobytes() == one_call[1][:7, 2:4].tobytes()
    e.reset()
    pcm, rep = e.run_cuts(sh["fr"], sh["ln"], (1, 3, 4))
    e.close()
    assert np.array_equal(pcm, one_call[0]) and rep.tobytes() == one_call[1].tobytes()


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------
def hostile_lists():
    """the four damaged frames in slot 0 and in slot 1 of a two-frame tick (3 for 80/147, 3 for 3/4), and in slot 1 of a one-frame tick,
    of the 44.1 kHz and the 32 kHz two-channel streams"""
    sh = A.shared()
    rng = np.random.default_rng(11)
    streams, lists = [], []
    for s, two, one in ((2, 3, 6), (4, 3, 4)):
        st = A.STREAMS[s]
        L, Mm = A.lm_of(st)
        assert A.want(two, L, Mm) == 2 and A.want(one, L, Mm) == 1
        for name, (b, n, _) in _damaged(sh["used"][s][5], rng).items():
            for tick, slot in ((two, 0), (two, 1), (one, 1)):
                sl = [list(p) for p in sh["lists"][s]]
                sl[tick][slot] = (b, n)
                streams.append(st); lists.append(sl)
    return streams, lists


def noise_calls(ns, stride):
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (A.NTICKS, ns, 2, stride), dtype=np.uint8)
    fr[1] = 0xff
    fr[2, :, :, :4] = [0xff, 0xfc, 0xf0, 0xff]
    ln = rng.integers(0, stride + 40, (A.NTICKS, ns, 2)).astype(np.int32)
    ln[3] = -5
    ln[6] = 10 ** 9
    ln[7, :, 0] = -(2 ** 31)
    return fr, ln


def test_hostile_input_is_clean_under_asan_ubsan(tmp_path):
    """the damaged sets, and noise under every kind of length (beyond the stride, negative) over the whole stream set, through the lane-loop
    build linked as a program with AddressSanitizer + UBSan (tests/emu/mp2_feed_down_san_main.cpp; its buffers are exactly as long as the
    data).  Clean, and the same reports and PCM as the plain build."""
    exe = A.build_san_driver()
    streams, lists = hostile_lists()
    e = A.FeedDownEmu(streams)
    fr, ln = A.slots_to_arrays(lists, e.stride)
    calls = [(fr[:1], ln[:1]), (fr[1:4], ln[1:4]), (fr[4:], ln[4:])]
    (rep, pcm), = A.run_san_driver(exe, tmp_path, streams, [calls])
    want_pcm, want_rep = e.run_cuts(fr, ln, (1, 3, 4))
    e.close()
    assert rep.tobytes() == want_rep.tobytes() and pcm.tobytes() == want_pcm.tobytes()
    e = A.FeedDownEmu(A.STREAMS)
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
    wanted, other = A.expected_status(A.STREAMS, ln)
    for s, st in enumerate(A.STREAMS[:6]):                       # noise decodes to silence: every fed stream's output is zeros
        assert not pcm[:, s][m[:, s]].any()
        for f in range(A.NTICKS):
            for j in range(2):
                stt = int(rep["status"][f, s, j])
                if not wanted[f, s, j]:
                    assert stt == int(other[f, s, j])
                else:
                    assert stt & D.BAD_MASK if ln[f, s, j] > 0 else stt == D.EMPTY
