"""The closing round of tl_allocate (csrc/mp2_alloc.h: key buckets, a histogram in the wave's LDS, one scan, the lane-by-lane pass for the cut's
bucket) on the GPU: the case set of tests/alloccutlib.py through the probe's allocation form (tlb_debug_probe_stage of the TEST library,
csrc/toolame_probe.hip: one wave per case, TlBlockShared in the workgroup's LDS, the histogram in the probe wave's LDS frame), one launch.
device == emulation (tests/emu/mp2_probe_emu.cpp), word for word, and == the reference's greedy loop restated event by event
(tests/probelib.py alloc_greedy).  tests/test_alloc_cut_emu.py has shown on the CPU that the set reaches the cut's hard cases."""
import pytest

import alloccutlib as A
import probelib as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def FI():
    import odr_audioenc_amd as M
    M.load_library()
    if not M.FAULT_LIB_PATH.exists():
        M.build()
    L = M.load_fault_library()
    P.bind_stage(L.tlb_debug_probe_stage)
    return L


def test_closing_round_device_is_emulation_is_oracle(FI):
    S = A.cut_set()
    rc, d_ba, d_left = A.run_probe(FI.tlb_debug_probe_stage, S)
    assert rc == 0
    rc, e_ba, e_left = A.run_probe(P.emu().probe_stage, S)
    assert rc == 0
    msg = P.stage_same("alloc", S, (d_ba, d_left), (e_ba, e_left))
    assert msg is None, msg
    msg = A.check(S, d_ba, d_left)
    assert msg is None, "device / oracle: " + msg
