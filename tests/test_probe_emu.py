"""The probe on the host (csrc/mp2_probe.h with -DTL_EMULATE, tests/emu/mp2_probe_emu.cpp): every device-path form of csrc/tl_libm.h against
this machine's libm, bit for bit, on the full argument sets of tests/probelib.py, and every cross-lane primitive of csrc/mp2_wave.h against
a numpy oracle written from the primitive's comment on the full case sets, and every shared stage helper of csrc/mp2_dbsum.h
(csrc/mp2_probe_stage.h) against an oracle written from the definition its comment states, on raw bits and integers -- and, one layer up, the
bit allocation alone (csrc/mp2_alloc.h: tl_allocate and tl_allocate_pair, the parameters `alloc` and `alloc_pair`) against the reference's
greedy loop restated event by event (tests/test_alloc_oracle_golden.py pins that restatement to the reference's taps), on sets built for
what whole frames seldom bring: exact ties, also between cells at different allocation levels, budgets that end on an event's cumulative
price or one bit short of it, refusals followed by cheaper admissions, units of a mono pair that stop at different times.  The set's coverage
conditions are checked from the oracle's trace.

That is what the GPU file (tests/test_probe_gpu.py) rests on: the argument sets lie inside the forms' stated domains (the probe refuses
anything else), and references, generators and oracles are right before a GPU is involved."""
import numpy as np
import pytest

import probelib as P

LIBM_FORMS = P.LIBM_FORMS


@pytest.fixture(scope="module")
def E():
    return P.emu()


@pytest.mark.parametrize("form,table", LIBM_FORMS, ids=["%s-%s" % (f, "lds" if t else "global") for f, t in LIBM_FORMS])
def test_libm_form_is_this_machines_libm(E, form, table):
    """the host half == glibc, bit for bit, on every argument of the set -- and the whole set is inside the form's domain (rc 0)"""
    a, b = P.arguments(form)
    assert a.size >= P.NRANDOM
    rc, r0, r1 = P.run_libm(E.probe_libm, form, table, a, b)
    assert rc == 0, "an argument of the set lies outside the form's stated domain"
    w0, w1 = P.glibc(form)
    for got, want in ((r0, w0), (r1, w1)):
        if want is None or form == "recip":                               # (no libm call to compare the refined reciprocal with: its check is the bound below)
            continue
        bad = P.same_bits(got, want)
        if bad.size and not P.libm_is_the_tables_libm():
            pytest.skip("another libm build than the one csrc/tl_libm_tables.inc names: %d of %d results differ from it" % (bad.size, a.size))
        assert not bad.size, P.report(form, a, b, got, want, bad)


def test_min_max_on_zeros_of_opposite_sign_keep_the_first_operand(E):
    """the documented exception of TLM_MIN_NN / TLM_MAX_NN (csrc/tl_libm.h): the host expressions return their FIRST operand for -0.0 against
    +0.0; the device's instructions order -0.0 below +0.0 (tests/test_probe_gpu.py pins that side).  No caller passes such a pair."""
    a, b = P.SIGNED_ZERO_TIES
    for form in ("min_nn", "max_nn"):
        rc, r0, _ = P.run_libm(E.probe_libm, form, 0, a, b)
        assert rc == 0 and not P.same_bits(r0, a).size


def test_seeds_of_the_host_half_meet_the_refinements_precondition(E):
    """... and the reciprocal refined from them is good to 2^-52 (the bounds: tests/probelib.py SEED_BOUND)"""
    for form in P.NOT_BIT_EQUAL:
        x, _ = P.arguments(form)
        rc, s, _ = P.run_libm(E.probe_libm, form, 0, x)
        assert rc == 0 and P.seed_error(form, x, s) <= P.SEED_BOUND[form]


def test_argument_checks(E):
    P.check_argument_checks(E.probe_libm, E.probe_wave, E.probe_stage)


@pytest.mark.parametrize("prim", list(P.PRIMS))
def test_wave_primitive_is_what_its_comment_says(E, prim):
    """the host half == the oracle on the full case set (TL_ROW16_MAX_F64: in lane 15 of each row, where its result is valid)"""
    w, in2 = P.wave_cases(prim)
    assert w.shape[0] >= P.NWAVES
    rc, out = P.run_wave(E.probe_wave, prim, w, in2)
    assert rc == 0
    want, lanes = P.wave_oracle(prim, w, in2)
    bad = np.argwhere(out[:, lanes] != want[:, lanes])
    assert not bad.size, "%s: %d words differ; first: case %d, row %s -> %s, want %s" % (
        prim, bad.shape[0], bad[0][0], [hex(int(x)) for x in np.ravel(w[bad[0][0]])], [hex(int(x)) for x in np.ravel(out[bad[0][0]])],
        [hex(int(x)) for x in np.ravel(want[bad[0][0]])])


@pytest.mark.parametrize("test", P.STAGE_TESTS)
def test_stage_helper_is_what_its_definition_says(E, test):
    """the stage helpers of csrc/mp2_dbsum.h through the emulation == the oracle on the full set, and the whole set inside the form's domain (rc 0)"""
    rc, S, out0, out1 = P.run_stage(E.probe_stage, test)
    assert rc == 0, "an argument of the set lies outside the form's stated domain"
    assert S["constructed"] > 0 and S["random"] >= 256
    msg = P.stage_check(test, S, out0, out1)
    assert msg is None, msg


@pytest.mark.parametrize("test", ("alloc", "alloc_pair"))
def test_allocation_sets_reach_the_hard_cases(E, test):
    """conditions on the SET, from the oracle's trace (tests/probelib.py alloc_coverage), none of them a measurement: each holds for at least
    ALLOC_COVER cases of the form of call -- an event with a tied minimum between different cells, one between cells at different allocation
    levels, a refusal followed by a later admission, bits left exactly 0, nothing admitted, every cell saturated, a joint pair's event won by
    channel 1 (tl_allocate), and for tl_allocate_pair: the units finish after different numbers of events, one unit stops short while the other
    runs to the end, both stop short, one unit has nothing while the other goes on.  Every table, both nch, every legal jsbound occur."""
    S = P.alloc_set(1 if test == "alloc_pair" else 0)
    cover = P.alloc_coverage(S)
    short = {k: v for k, v in cover.items() if v < P.ALLOC_COVER}
    assert not short, "%s: too few cases for %s (all: %s)" % (test, short, cover)
    T = P._alloc_tables()
    seen = set(zip(S["tab"].tolist(), S["nch"].tolist(), S["jsb"].tolist()))
    for t in range(5):
        want = {(t, 1, int(T["sblimit"][t]))} | (set() if test == "alloc_pair" else {(t, 2, j) for j in (4, 8, 12, 16, int(T["sblimit"][t]))})
        assert want <= seen, (t, sorted(want - seen))
    assert S["tab"].size <= 8192
