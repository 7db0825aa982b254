"""Feed concealment on ADAPTED and DOWN feeds (csrc/mp2_conceal_conv.h between csrc/mp2_feed_adapt.h / csrc/mp2_feed_down.h's decode and
their resampler or decimator) on the lane-loop emulation, without a GPU.  The property: the PCM the ingest receives is, bit for bit, what
the chain "strict concealed feed at the feed's own rate and channel count over the WANTED slots, the channel map, the resampler or
decimator" gives (tests/concealconvlib.py composes it from conceallib, feedadaptlib / resamplelib and feeddownlib / decimatelib), and the
record is that strict feed's; neither depends on how the ticks are cut into calls.  Seven feed cases; conceallib's scenarios over at least
sixteen wanted slots and the ones only a schedule with unwanted slots has; guard words around the source plane and G; the hostile slots
once more as a program linked with AddressSanitizer + UBSan.  The emulation is compiled by concealconvlib into a temporary directory."""
import shutil

import numpy as np
import pytest

import concealconvlib as V
import conceallib as K
import declib as D
import feedadaptlib as FA
import feeddownlib as FD

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")

_RUNS = {}


def run_case(ci, cut="12"):
    """case ci's scenario batch under one cut, once: (rows, frames, lens, pcm, reports, records, guard)"""
    if (ci, cut) not in _RUNS:
        case = V.CASES[ci]
        rows = V.scenario_batch(ci)
        e = V.ConcealConvEmu(rows)
        fr, ln = V.batch_arrays(rows, e.stride)
        pcm, rep, rec = e.run_cut(fr, ln, V.cuts_of(case)[cut])
        guard = e.guard_ok()
        e.close()
        _RUNS[(ci, cut)] = (rows, fr, ln, pcm, rep, rec, guard)
    return _RUNS[(ci, cut)]


def test_the_cases_scenarios_and_cuts_are_the_ones_asked_for():
    assert [(k, f[0], f[1], e[0], e[1]) for k, f, e in V.CASES] == [
        ("adapt", 32000, "s", 48000, "s"), ("adapt", 44100, "s", 48000, "m"), ("adapt", 48000, "m", 48000, "s"), ("adapt", 16000, "s", 24000, "s"),
        ("down", 48000, "s", 24000, "s"), ("down", 32000, "s", 24000, "s"), ("down", 44100, "m", 24000, "m")]
    # the schedules: the first unwanted tick is tick 2 at 3/2 and tick 12 at 160/147; the first one-frame tick is tick 1 at 3/4 and tick 6 at 80/147
    first = [next((t for t in range(40) if V.feed_want_at(c, t) < V.slots_per_tick(c)), None) for c in V.CASES]
    assert first == [2, 12, None, 2, None, 1, 6]
    for ci, case in enumerate(V.CASES):
        nt, nw, w = V.schedule(case)
        assert nw >= 16 and nw == sum(w) and len(w) == nt
        sc = {name: (hold, step, ways, fill) for name, hold, step, ways, fill in V.scenarios(case)}
        assert all(len(v[2]) == nw for v in sc.values())
        assert {(v[0], v[1]) for v in sc.values()} == {(h, s) for h in (1, 4, 16) for s in (1, 3, 21)}
        assert {"empty", "crc", "sync", "trunc", "random", "bitrate", "alloc"} <= set(sc["ways"][2])
        assert [x is not None for x in sc["alternating"][2][:4]] == [False, True, False, True] and [x is not None for x in sc["even"][2][:4]] == [True, False, True, False]
        u, a = V.first_short_tick(case)
        lost_in, lost_bh = ([x is not None for x in sc[n][2]] for n in ("inside", "behind"))
        assert lost_in[a - 2:a + 2] == [True] * 4 and sum(lost_in) == 4 and sc["inside"][3]       # the unwanted slot between a - 1 and a carries bytes
        assert lost_bh[a - 3:a + 1] == [True] * 3 + [False] and sum(lost_bh) == 3
        cuts = V.cuts_of(case)
        assert all(sum(c) == nt for c in cuts.values()) and set(K.CUTS) <= set(cuts)
        if u is not None:
            assert a >= 4 and w[u] < V.slots_per_tick(case) and cuts["unwanted"][:2] == [u, 1]   # a call boundary either side of tick u
            rows = V.scenario_batch(ci)
            by = {r["name"]: r for r in rows}
            tick = by["inside"]["ticks"][u]
            assert (tick if V.slots_per_tick(case) == 1 else tick[1])[1] > 0                      # bytes in the unwanted slot
    # a down-feed tick that loses slot 0 but not slot 1, and one that loses slot 1 but not slot 0 (1/2: slot j of every tick is wanted slot 2 t + j)
    assert all(V.feed_want_at(V.CASES[4], t) == 2 for t in range(9))


@pytest.mark.parametrize("ci", range(len(V.CASES)), ids=V.CASE_IDS)
def test_every_scenario_equals_the_chain(ci):
    """every PCM sample and every record word, the cut of conceallib's twelve; the reports say lost exactly where the scenario lost a wanted
    slot, and EMPTY (| UNWANTED where it carries bytes) for every unwanted one"""
    rows, _, _, pcm, rep, rec, guard = run_case(ci)
    V.check_rows(rows, pcm, rep, rec, "12")
    assert guard
    by = {r["name"]: s for s, r in enumerate(rows)}
    nw = V.schedule(V.CASES[ci])[1]
    assert int(rec[by["none"]]["frames"]) == nw and int(rec[by["none"]]["passed"]) == nw - 2      # frames counts wanted slots (the tail loses two)
    assert int(rec[by["inside"]]["concealed"]) == 4 and int(rec[by["inside"]]["longest"]) == 4 and int(rec[by["inside"]]["runs"]) == 1
    assert int(rec[by["behind"]]["concealed"]) == 3 and int(rec[by["behind"]]["run"]) == 0
    assert int(rec[by["hold+3"]]["muted"]) == 2 and int(rec[by["hold+1"]]["muted"]) == 0
    # concealment changes what comes out: the same losses without it give other samples
    none, one = by["none"], by["one"]
    assert not np.array_equal(pcm[:, none], pcm[:, one])


@pytest.mark.parametrize("ci", range(len(V.CASES)), ids=V.CASE_IDS)
def test_every_cut_gives_the_same_bytes_and_records(ci):
    """calls of 1, 2, 3, 4, 6 and 12 ticks and 5 + 7 over and over, and a call boundary either side of an unwanted tick: loss runs that cross
    a boundary, G from the carry, runs counted in wanted slots across calls that hold none"""
    _, _, _, pcm, rep, rec, _ = run_case(ci)
    for cut in V.cuts_of(V.CASES[ci]):
        _, _, _, p, r, c, guard = run_case(ci, cut)
        assert p.tobytes() == pcm.tobytes() and r.tobytes() == rep.tobytes() and c.tobytes() == rec.tobytes(), cut
        assert guard, cut


@pytest.mark.parametrize("ci", (1, 5), ids=[V.CASE_IDS[1], V.CASE_IDS[5]])
def test_streams_without_concealment_are_todays(ci):
    """the fed stream without concealment beside the others, and a batch in which nobody has it on: the bytes of the path's own emulation
    (tests/emu/mp2_feed_emu.cpp, tests/emu/mp2_feed_down_emu.cpp), which knows nothing of concealment; zero records"""
    case = V.CASES[ci]
    rows, fr, ln, pcm, rep, rec, _ = run_case(ci)
    s = [r["name"] for r in rows].index("unconcealed")
    if case[0] == "down":
        e = FD.FeedDownEmu([dict(feed=case[1] if r["fcfg"] else None, mode=case[2][1]) for r in rows])
    else:
        e = FA.FeedAdaptEmu([dict(feed=case[1] if r["fcfg"] else None, enc=case[2], adapt=True) for r in rows])
    p, q = e.decode(fr, ln)
    e.close()
    assert np.array_equal(q, rep)                                # reports are unchanged by concealment, for every stream
    assert np.array_equal(p[:, s], pcm[:, s]) and not rec[s].tobytes().strip(b"\0")
    none = [r["name"] for r in rows].index("none")
    w = V.schedule(case)[2]
    t13 = next(t for t in range(len(w)) if sum(w[:t + 1]) > 13)  # the tick of the first lost wanted slot of "none" (its tail's)
    assert t13 >= 5 and np.array_equal(p[:t13, none], pcm[:t13, none])      # concealment on, nothing lost yet: the path's bytes
    assert (pcm[:, -1] == V.POISON).all() and not rec[-1].tobytes().strip(b"\0")
    off = [dict(r, hold=0, step=0) for r in rows]
    e = V.ConcealConvEmu(off)
    p2, q2 = e.decode(fr, ln)
    assert e.guard_ok() and not e.records().tobytes().strip(b"\0")
    e.close()
    assert np.array_equal(p2, p) and np.array_equal(q2, q)


def test_a_reset_forgets_g_run_and_record():
    """after a reset a stream's run starts from a reset's state: the second run's bytes and records are the first's"""
    ci = 3
    case = V.CASES[ci]
    rows, fr, ln, pcm, rep, rec, _ = run_case(ci)
    e = V.ConcealConvEmu(rows)
    e.run_cut(fr[:7], ln[:7], [3, 4])
    e.reset()
    assert not e.records().tobytes().strip(b"\0")
    p, r, c = e.run_cut(fr, ln, [fr.shape[0]])
    e.close()
    assert p.tobytes() == pcm.tobytes() and c.tobytes() == rec.tobytes()


def test_hostile_losses_are_clean_under_asan_ubsan(tmp_path):
    """the scenario batches with the hostile lost slots (feedlib.hostile_inputs' damage, in "ways"), cut 5 + 7, through the lane-loop build
    linked as a program with AddressSanitizer + UBSan (tests/emu/mp2_conceal_conv_san_main.cpp: its buffers are exactly as long as the data,
    the plane and the G slots have poisoned neighbours).  Clean, and the same bytes as the plain build's, which the tests above have checked."""
    exe = V.build_san_driver()
    for ci in (1, 2, 4, 5):                                      # 160/147 with the map, 1/1 one channel to two, 1/2 (two wanted slots a tick), 3/4
        case = V.CASES[ci]
        rows, fr, ln, pcm, rep, rec, _ = run_case(ci)
        calls, at = [], 0
        for n in V.cuts_of(case)["5+7"]:
            calls.append((fr[at:at + n], ln[at:at + n])); at += n
        out, got_rec, guard = V.run_san_driver(exe, tmp_path, rows, calls)
        assert guard
        assert np.concatenate([o[0] for o in out]).tobytes() == rep.tobytes() and np.concatenate([o[1] for o in out]).tobytes() == pcm.tobytes(), V.CASE_IDS[ci]
        assert got_rec.tobytes() == rec.tobytes()
