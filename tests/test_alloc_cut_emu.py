"""The closing round of tl_allocate (csrc/mp2_alloc.h) on the CPU: the round that does not fit as a whole is cut by key buckets -- a histogram
of the round's prices over at most 64 buckets of its key window, one scan, the lane-by-lane pass for the one bucket the cut falls into.  The
emulation (the same text with -DTL_EMULATE, tests/emu/mp2_alloc_cut_emu.cpp) against the reference's greedy loop restated event by event
(tests/probelib.py alloc_greedy), word for word, on a set built for that round (tests/alloccutlib.py): cuts in the first and in the last
occupied bucket, budgets on a bucket's running sum and one bit short of it, rounds whose keys share one bucket or are all equal, a closing
round that is the first round, windows over negative and positive MNR, joint pairs tied at the cut, rounds of 1 and of 54 events.

The set's coverage is asserted from the path counters the emulation keeps per case (TL_DBG_ALLOC: which branch ran, how many events were left
to the lane-by-lane pass), and four mutants of the bucket pass must each fail the comparison."""
import numpy as np
import pytest

import alloccutlib as A
import probelib as P


@pytest.fixture(scope="module")
def S():
    return A.cut_set()


@pytest.fixture(scope="module")
def ran(S):
    rc, ba, left, st = A.run_emu(A.lib("cut"), S)
    assert rc == 0
    return ba, left, st


def test_emulation_is_the_greedy_loop_word_for_word(S, ran):
    ba, left, st = ran
    msg = A.check(S, ba, left)
    assert msg is None, "emulation / oracle: " + msg
    msg = A.check_rule(S, st)
    assert msg is None, msg


def test_the_probes_emulation_agrees(S, ran):
    """tests/emu/mp2_probe_emu.cpp (what the GPU test compares the device with) runs the same text without counters"""
    rc, ba, left = A.run_probe(P.emu().probe_stage, S)
    assert rc == 0 and (ba == ran[0]).all() and (left == ran[1]).all()


def test_lane_by_lane_build_agrees(S, ran):
    """-DTL_CUT_PASSES=0 is the lane-by-lane pass alone, the loop before the buckets: the same words, and every event left to that pass"""
    rc, ba, left, st = A.run_emu(A.lib("serial"), S)
    assert rc == 0 and (ba == ran[0]).all() and (left == ran[1]).all()
    assert (st[:, A.K["SERIAL"]] == st[:, A.K["EVENTS"]]).all() and not st[:, A.K["PASS1"]].any()
    assert A.check_rule(S, st) is None


def test_set_reaches_the_hard_cases(S, ran):
    """at least 32 cases of each kind (the convention of tests/probelib.py ALLOC_COVER), every closing round the partial-round branch, no key
    outside the window [the round before's smallest second key, this round's) the buckets are laid over, and never more than two passes"""
    _, _, st = ran
    L = A.lib("cut")
    cover = A.coverage(S, st, L.alloc_cut_serial_limit())
    print("%d cases; %s" % (st.shape[0], cover))
    short = {k: v for k, v in cover.items() if v < A.COVER}
    assert not short, "too few cases for %s (all: %s)" % (short, cover)
    assert set(A.KINDS) <= set(cover)
    assert (st[:, A.K["PARTIAL"]] == 1).all(), "a case whose closing round fits as a whole: %s" % S["names"][int(np.flatnonzero(st[:, A.K["PARTIAL"]] != 1)[0])]
    assert not st[:, A.K["BELOW"]].any(), "a key outside the window"
    assert (st[:, A.K["PASS1"]] <= 1).all() and (st[:, A.K["PASS2"]] <= st[:, A.K["PASS1"]]).all()
    # a pass never leaves MORE to the lane-by-lane pass, and a cut that ran leaves the cut bucket alone
    assert (st[:, A.K["SERIAL"]] <= st[:, A.K["EVENTS"]]).all()
    seen = set(zip(S["tab"].tolist(), S["nch"].tolist(), S["jsb"].tolist()))
    T = P._alloc_tables()
    for t in range(5):
        want = {(t, 1, int(T["sblimit"][t]))} | {(t, 2, j) for j in (4, 8, 12, 16, int(T["sblimit"][t]))}
        assert want <= seen, (t, sorted(want - seen))
    assert np.abs(S["smr"]).max() <= 1000.0


@pytest.mark.parametrize("mutant", sorted(A.MUTANTS))
def test_mutant_fails(S, mutant):
    """each mutant fails what test_emulation_is_the_greedy_loop_word_for_word asserts: the words where it admits too much, the rule's count where
    it cuts the round short (the event-by-event loop then repairs the words)"""
    rc, ba, left, st = A.run_emu(A.lib(mutant), S)
    assert rc == 0
    words, rule = A.check(S, ba, left), A.check_rule(S, st)
    print(mutant, "| words:", words, "| rule:", rule)
    assert words is not None or rule is not None, "the set does not see: " + A.MUTANTS[mutant]
