"""The probe on the GPU (csrc/toolame_probe.hip in the fault-injection TEST library, csrc/tlb_debug.h: tlb_debug_probe_libm / _wave): the
DEVICE halves of csrc/tl_libm.h and of csrc/mp2_wave.h's cross-lane primitives, one by one, on the argument and case sets of
tests/probelib.py -- hardware reciprocal / reciprocal-square-root seeds, inline v_fma_f64 / v_min_f64 / v_max_f64, tables as device globals,
as LDS copies and rearranged (TL_SCT), DPP ladders, permlane swaps, ballots -- and (tlb_debug_probe_stage, csrc/mp2_probe_stage.h) the shared stage helpers
of csrc/mp2_dbsum.h as the device build compiles them: dB sums, masking terms, masker spans, row minimum, allocation key, scalefactor index, exact
division, the bit writer (64 lanes' atomicOr into one LDS frame) and the CRC step -- and, one layer up, the bit allocation alone (csrc/mp2_alloc.h:
tl_allocate and tl_allocate_pair, one wave per case, TlBlockShared in the workgroup's LDS as the frame kernel keeps it) against the reference's greedy
loop restated event by event, on sets of ties, budget edges and refusals that whole frames seldom bring (the parameters `alloc` and `alloc_pair`).

The hard assertion is device == emulation (tests/emu/mp2_probe_emu.cpp, the host halves through the same text), bit for bit: it does not
depend on this machine's libm.  tests/test_probe_emu.py has shown the emulation equal to glibc and to the oracles on the same sets, and the
sets inside the forms' domains; the probe refuses every argument outside them on the host, so nothing here provokes the device."""
import datetime
import os
from pathlib import Path

import numpy as np
import pytest

import probelib as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def FI(M):
    if not M.FAULT_LIB_PATH.exists():
        M.build()
    L = M.load_fault_library()
    P.bind_probe(L.tlb_debug_probe_libm, L.tlb_debug_probe_wave)
    P.bind_stage(L.tlb_debug_probe_stage)
    return L


@pytest.fixture(scope="module")
def E():
    return P.emu()


BIT_EQUAL = [(f, t) for f, t in P.LIBM_FORMS if f not in P.NOT_BIT_EQUAL]


@pytest.mark.parametrize("form,table", BIT_EQUAL, ids=["%s-%s" % (f, "lds" if t else "global") for f, t in BIT_EQUAL])
def test_libm_form_device_is_emulation_is_glibc(FI, E, form, table):
    a, b = P.arguments(form)
    rc, d0, d1 = P.run_libm(FI.tlb_debug_probe_libm, form, table, a, b)
    assert rc == 0
    rc, e0, e1 = P.run_libm(E.probe_libm, form, table, a, b)
    assert rc == 0
    for got, want in ((d0, e0), (d1, e1)):                                # the hard assertion
        if want is not None:
            bad = P.same_bits(got, want)
            assert not bad.size, "device / emulation: " + P.report(form, a, b, got, want, bad)
    w0, w1 = P.glibc(form)
    for got, want in ((d0, w0), (d1, w1)):
        if want is not None:
            bad = P.same_bits(got, want)
            if bad.size and not P.libm_is_the_tables_libm():
                pytest.skip("another libm build than the one csrc/tl_libm_tables.inc names: %d of %d results differ from it" % (bad.size, a.size))
            assert not bad.size, "device / glibc: " + P.report(form, a, b, got, want, bad)


def test_min_max_on_zeros_of_opposite_sign_order_them(FI):
    """the documented exception of TLM_MIN_NN / TLM_MAX_NN (csrc/tl_libm.h), the device's side: v_min_f64 / v_max_f64 order -0.0 below +0.0
    whichever operand it is; the host expressions keep their first operand (tests/test_probe_emu.py).  No caller passes such a pair."""
    a, b = P.SIGNED_ZERO_TIES
    rc, lo, _ = P.run_libm(FI.tlb_debug_probe_libm, "min_nn", 0, a, b)
    assert rc == 0 and not P.same_bits(lo, np.array([-0.0, -0.0])).size
    rc, hi, _ = P.run_libm(FI.tlb_debug_probe_libm, "max_nn", 0, a, b)
    assert rc == 0 and not P.same_bits(hi, np.array([0.0, 0.0])).size


def test_hardware_seeds_meet_the_refinements_precondition(FI):
    """v_rcp_f64 / v_rsq_f64 as they are: the largest relative error over the sets is below 2^-20, the precondition csrc/tl_libm.h states for
    tlm_recip_from / tlm_sqrt_from and tools/libm_agree.cpp shows convergence from -- and the reciprocal tlm_recip_from makes of the seed is good
    to 2^-52 (tests/probelib.py SEED_BOUND: the one check that sees a refinement step go missing; the quotients stay correctly rounded without it).
    The measured maxima are printed, and written to the file TL_PROBE_SEEDS_OUT names (profiles/probe_seeds.txt is such a record)."""
    lines = ["largest relative error of the hardware seeds of csrc/tl_libm.h and of the refined reciprocal (tests/test_probe_gpu.py, %s)" % datetime.date.today().isoformat()]
    worst = {}
    for form, what in (("rcp_seed", "v_rcp_f64       max |seed d - 1|      "), ("rsq_seed", "v_rsq_f64       max |seed^2 x - 1| / 2"), ("recip", "tlm_recip_from  max |r d - 1|         ")):
        x, _ = P.arguments(form)
        rc, s, _ = P.run_libm(FI.tlb_debug_probe_libm, form, 0, x)
        assert rc == 0
        worst[form] = P.seed_error(form, x, s)
        lines.append("%s over %d arguments in [2^-500, 2^500]: %.6e = 2^%.2f (bound 2^%d)" % (what, x.size, worst[form], np.log2(worst[form]), round(np.log2(P.SEED_BOUND[form]))))
    print("\n".join(lines))
    if os.environ.get("TL_PROBE_SEEDS_OUT"):
        Path(os.environ["TL_PROBE_SEEDS_OUT"]).write_text("\n".join(lines) + "\n")
    for form in worst:
        assert worst[form] <= P.SEED_BOUND[form], lines


def test_argument_checks(FI):
    """outside a form's domain, unknown form, n = 0, a missing pointer: 18 each, before anything is queued; then a good call with the right bits"""
    P.check_argument_checks(FI.tlb_debug_probe_libm, FI.tlb_debug_probe_wave, FI.tlb_debug_probe_stage)


@pytest.mark.parametrize("prim", list(P.PRIMS))
def test_wave_primitive_device_is_emulation_is_oracle(FI, E, prim):
    w, in2 = P.wave_cases(prim)
    rc, dev = P.run_wave(FI.tlb_debug_probe_wave, prim, w, in2)
    assert rc == 0
    rc, emu = P.run_wave(E.probe_wave, prim, w, in2)
    assert rc == 0
    want, lanes = P.wave_oracle(prim, w, in2)
    for name, ref in (("emulation", emu), ("oracle", want)):
        bad = np.argwhere(dev[:, lanes] != ref[:, lanes])
        assert not bad.size, "%s, device / %s: %d words differ; first: case %d, row %s -> %s, want %s" % (
            prim, name, bad.shape[0], bad[0][0], [hex(int(x)) for x in np.ravel(w[bad[0][0]])], [hex(int(x)) for x in np.ravel(dev[bad[0][0]])],
            [hex(int(x)) for x in np.ravel(ref[bad[0][0]])])


@pytest.mark.parametrize("test", P.STAGE_TESTS)
def test_stage_helper_device_is_emulation_is_oracle(FI, E, test):
    """one launch per form: every output word of the device == the emulation's (the hard assertion), and == the oracle written from the definition"""
    rc, S, d0, d1 = P.run_stage(FI.tlb_debug_probe_stage, test)
    assert rc == 0
    rc, _, e0, e1 = P.run_stage(E.probe_stage, test)
    assert rc == 0
    msg = P.stage_same(test, S, (d0, d1), (e0, e1))
    assert msg is None, msg
    msg = P.stage_check(test, S, d0, d1)
    assert msg is None, "device / oracle: " + msg
