"""Feed concealment (csrc/mp2_conceal.h behind csrc/mp2_feed.h) on the lane-loop emulation, without a GPU: every loss scenario against the
oracle (tests/conceallib.py, a sequential loop over the definition), every cut of the twelve slots into calls against the uncut run, a
property of the attenuation that does not go through the oracle, the record's arithmetic on a hand-written status sequence, and the
whole as a program linked with AddressSanitizer + UBSan.  The emulation is compiled by this module into a temporary directory."""
import shutil

import numpy as np
import pytest

import conceallib as K
import declib as D
import feedlib as F

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")

CASE_IDS = [f"{fs // 1000}k_{mode}_{kbps}" for fs, mode, kbps, _ in K.CASES]


@pytest.fixture(scope="module")
def so(tmp_path_factory):
    return K.build_emu(tmp_path_factory.mktemp("concealemu"))


_RUNS = {}


def run_case(so, i, cut="12"):
    """case i's scenario batch under one cut, once: (rows, frames, lens, pcm, reports, records, guard)"""
    if (i, cut) not in _RUNS:
        rows = K.scenario_batch([i])
        e = K.ConcealEmu(so, rows)
        fr, ln = K.batch_arrays(rows, e.stride)
        pcm, rep, rec = e.run_cut(fr, ln, K.CUTS[cut])
        guard = e.guard_ok()
        e.close()
        _RUNS[(i, cut)] = (rows, fr, ln, pcm, rep, rec, guard)
    return _RUNS[(i, cut)]


def test_the_scenarios_are_the_ones_asked_for():
    assert [c[:3] for c in K.CASES] == [(48000, "s", 192), (48000, "j", 128), (48000, "d", 64), (48000, "m", 64), (44100, "s", 128), (32000, "s", 384)]
    sc = {name: (hold, step, ways) for name, hold, step, ways in K.scenarios()}
    lost = {n: [w is not None for w in v[2]] for n, v in sc.items()}
    assert all(len(v) == K.NSLOTS for v in lost.values())
    assert sum(lost["none"]) == 0 and sum(lost["one"]) == 1
    assert lost["hold"] == [False] * 2 + [True] * 4 + [False] * 6 and sum(lost["hold+1"]) == 5 and sum(lost["hold+3"]) == 7
    assert lost["first"][:3] == [True, True, False] and lost["alternating"] == [False, True] * 6
    assert lost["two_runs"] == [False, True, True, True, False, True, True, True, False, False, False, False]
    assert {"empty", "crc", "sync", "trunc", "long", "random", "bitrate", "alloc"} <= set(sc["ways"][2])
    assert {(h, s) for _, h, s, _ in K.scenarios()} == {(h, s) for h in (1, 4, 16) for s in (1, 3, 21)}
    rows = K.scenario_batch([3])
    assert rows[-1]["fcfg"] is None and rows[-3]["hold"] == 0 and any(rows[-3]["lost"]) and rows[-3]["fcfg"]["channels"] == 1


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=CASE_IDS)
def test_every_scenario_equals_the_oracle(so, i):
    """every PCM sample and every record word, one call of twelve slots; the reports say lost exactly where the scenario lost a slot"""
    rows, _, _, pcm, rep, rec, guard = run_case(so, i)
    K.check_rows(rows, pcm, rep, rec, "12")
    assert guard
    by = {r["name"]: s for s, r in enumerate(rows)}
    assert pcm[5, by["one"], :1152].any()                        # a concealed slot is audio, not silence
    assert not pcm[0, by["first"], :1152 * rows[0]["fcfg"]["channels"]].any()     # no G yet: silence
    assert int(rec[by["hold+3"]]["muted"]) == 2 and int(rec[by["hold+1"]]["concealed"]) == 5 and int(rec[by["hold+1"]]["muted"]) == 0


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=CASE_IDS)
def test_every_cut_gives_the_same_bytes_and_records(so, i):
    """launches of 1, 2, 3, 4, 6 and 12 frames and 5 + 7: loss runs that cross a launch boundary, G from the carry, the window reaching slot 0"""
    _, _, _, pcm, rep, rec, _ = run_case(so, i)
    for cut in K.CUTS:
        _, _, _, p, r, c, guard = run_case(so, i, cut)
        assert p.tobytes() == pcm.tobytes() and r.tobytes() == rep.tobytes() and c.tobytes() == rec.tobytes(), cut
        assert guard, cut


def test_streams_without_concealment_are_the_feeds_own(so):
    """the fed stream without concealment: feedlib.numpy_feed_pcm's bytes; the stream without a feed keeps POISON"""
    rows, fr, ln, pcm, rep, rec, _ = run_case(so, 0)
    s = [r["name"] for r in rows].index("unconcealed")
    lost = rows[s]["lost"]
    want = F.numpy_feed_pcm([None if gone else bytes(b)[:n] for (b, n), gone in zip(rows[s]["slots"], lost)], rows[s]["fcfg"])
    assert np.array_equal(pcm[:, s], want) and not pcm[np.array(lost), s].any() and not rec[s].tobytes().strip(b"\0")
    assert rows[-1]["fcfg"] is None and (pcm[:, -1] == K.POISON).all() and not rec[-1].tobytes().strip(b"\0")
    # ... and it is what the feed emulation alone gives for the whole batch's untouched streams
    e = F.FeedEmu(F.build_emu(so.parent), [r["fcfg"] for r in rows])
    p, q = e.decode(fr, ln)
    e.close()
    assert np.array_equal(p[:, s], pcm[:, s]) and np.array_equal(q, rep)
    none = [r["name"] for r in rows].index("none")
    assert np.array_equal(p[:, none], pcm[:, none])              # concealment on, nothing lost: the feed's bytes


def test_a_repeat_is_the_good_frame_halved_per_step_of_three(so):
    """not through the oracle's concealment code.  step = 3 and a lost slot with k <= hold: samples 480..1151 of each channel satisfy
    |2^k y[i] - g[i]| <= 2^(k - 1) + 1 with g the plain decode of the good frame -- output vectors 15..35 reach back no further than the
    frame's own vector 0, and an index raised by 3 is a factor 1/2 to 1e-14; y is rounded to half a step (2^(k - 1) after the scaling) and
    g to half a step."""
    case = K.CASES[0]
    fcfg = F.feed_cfg_of(case)
    frames = F.oracle_frames(case, F.case_pcm(0, case, K.NSLOTS) // 4)
    rows = [dict(fcfg=fcfg, hold=4, step=3), dict(fcfg=fcfg, hold=0, step=0)]
    good = [(b, len(b)) for b in frames]
    lossy = list(good)
    for f in (4, 5, 6, 7):
        lossy[f] = (b"", 0)
    e = K.ConcealEmu(so, rows)
    fr, ln = F.slots_to_arrays([lossy, good], e.stride)
    pcm, rep = e.decode(fr, ln)
    e.close()
    g = pcm[3, 1].astype(np.int64).reshape(1152, 2)
    assert np.array_equal(pcm[3, 0], pcm[3, 1])
    assert 1000 < np.abs(g).max() < 16384                        # audio below half scale: g does not saturate
    for k in (1, 2, 3, 4):
        y = pcm[3 + k, 0].astype(np.int64).reshape(1152, 2)
        d = np.abs((y[480:] << k) - g[480:])
        print(f"k = {k}: max |2^k y - g| = {int(d.max())}, bound {2 ** (k - 1) + 1}")
        assert d.max() <= 2 ** (k - 1) + 1, k
        assert np.abs(y[480:]).max() > 30


def test_record_arithmetic_on_a_hand_written_sequence(so):
    """no audio: the carry alone.  L = lost, P = passes"""
    P, P2, L1, L2, L3 = 0, D.SCFCRC_UNCHECKED, D.EMPTY, D.BAD_CRC16, D.BAD_SYNC | D.OVERRUN
    #      0   1   2  3   4   5   6   7   8   9   10  11 12
    seq = [L1, L2, P, L3, P2, L1, L1, L2, L3, L1, P, P, L2]
    # hold 2: slots 0, 1 muted (no G); 3 concealed; 5, 6 and the ring-out frame 7 concealed, 8, 9 muted; 12 concealed
    want = dict(frames=13, passed=4, concealed=5, muted=4, runs=4, longest=5, run=1, offset=5)
    for cut in ([13], [1] * 13, [6, 7], [8, 5], [9, 4], [2, 11]):
        rec = K.emu_fold(so, 2, 5, seq, cut)
        assert {n: int(rec[n]) for n in K.RECORD_FIELDS} == want, cut
    rec = K.emu_fold(so, 2, 5, [P, L1, L1, L1, L1], [5])
    assert (int(rec["run"]), int(rec["offset"]), int(rec["concealed"]), int(rec["muted"])) == (4, K.MUTE, 3, 1)
    rec = K.emu_fold(so, 2, 5, [P, L1, L1], [3])
    assert (int(rec["run"]), int(rec["offset"])) == (2, 10)
    # more slots than lanes in one call, and the same cut at and around the 64th
    long = [P] + [L1] * 69
    want = dict(frames=70, passed=1, concealed=17, muted=52, runs=1, longest=69, run=69, offset=K.MUTE)
    for cut in ([70], [1, 69], [64, 6], [63, 7], [65, 5], [10] * 7):
        rec = K.emu_fold(so, 16, 1, long, cut)
        assert {n: int(rec[n]) for n in K.RECORD_FIELDS} == want, cut
    for hold in (1, 2, 16):
        rng = np.random.default_rng(hold)
        lost = (rng.random(200) < 0.6).tolist()
        rec = K.emu_fold(so, hold, 3, [L1 if x else P for x in lost], [200])
        assert rec == K.oracle_record(lost, hold, 3)


def test_hostile_losses_are_clean_under_asan_ubsan(tmp_path, so):
    """the scenario batches with the hostile lost slots, cut 5 + 7, through the lane-loop build linked as a program with AddressSanitizer +
    UBSan (tests/emu/mp2_conceal_san_main.cpp: its buffers are exactly as long as the data, the G slots have poisoned neighbours).  Clean,
    and the same bytes as the plain build's, which the tests above have checked."""
    exe = K.build_san_driver(tmp_path)
    for i in (1, 4, 5):
        rows, fr, ln, pcm, rep, rec, _ = run_case(so, i)
        calls = [(fr[:5], ln[:5]), (fr[5:], ln[5:])]
        out, got_rec, guard = K.run_san_driver(exe, tmp_path, rows, calls)
        assert guard
        assert np.concatenate([o[0] for o in out]).tobytes() == rep.tobytes() and np.concatenate([o[1] for o in out]).tobytes() == pcm.tobytes(), CASE_IDS[i]
        assert got_rec.tobytes() == rec.tobytes()
