"""The frame kernels' one-instruction maxima and minima (csrc/tl_libm.h: tlm_max_gt, tlm_min_lt, tlm_maxabs_gt, tlm_maxabs2_gt, tlm_fmax_k;
used by csrc/mp2_pack.h and csrc/mp2_psy13.h).  On the device each is one v_max_f64 / v_min_f64, which differs from the statement it replaces
only for a NaN operand or for zeros of opposite sign; in the emulation each IS that statement and reports its operand pair to TL_DBG_MINMAX.
So two things are checked here, CPU only: the emulation still equals the oracle byte for byte on every group of tests/minmaxlib.py, and the
hook's count of unsafe pairs (emu_minmax_stats) stays at zero while every converted site is seen to have run.  What the instruction itself
does with these inputs is the GPU half's business (tests/test_minmax_forms_gpu.py)."""
import ctypes

import numpy as np
import pytest

import emulib as E
import minmaxlib as X


def _stats():
    L = E.lib()
    a = (ctypes.c_long * (2 + 2 * len(X.SITES)))()
    L.emu_minmax_stats(a)
    return np.array(list(a), dtype=np.int64)


@pytest.mark.parametrize("gi", range(len(X.groups())), ids=[g[0] for g in X.groups()])
def test_emulation_equals_oracle_and_no_pair_is_unsafe(gi):
    name, cfg, pcms = X.groups()[gi]
    want = X.oracle_bytes(gi)
    b = E.EmuBatch([cfg] * len(pcms))
    s0 = _stats()
    got, _ = b.encode(np.stack(pcms, axis=1))
    tail = b.flush()
    pairs_run = b.pair_units()
    b.close()
    d = _stats() - s0
    per = {s: (int(d[2 + 2 * k]), int(d[3 + 2 * k])) for k, s in enumerate(X.SITES)}
    print(name, "operand pairs (reported, unsafe) by site:", per)
    for s in range(len(pcms)):
        assert got[s] + tail[s] == want[s], (name, s)
    assert d[0] == 0, per                                            # no NaN, no zeros of opposite sign at any converted site
    assert d[1] == sum(p for p, _ in per.values()) and d[1] > 0
    units = len(pcms) * X.NFRAMES
    psy, mode = cfg["psy"], cfg["mode"]
    if mode == "m":
        assert pairs_run == X.NFRAMES                                # the two mono streams shared a wave: tl_encode_pair
    # scalefactor maxima: eleven pairs per granule and live (subband, channel) cell, whichever encoder ran
    assert per["scf"][0] > 0 and per["scf"][0] % (11 * 3) == 0
    assert (per["jscf"][0] > 0) == (mode == "j")
    assert (per["smr"][0] > 0) == (psy in (1, 3))
    assert (per["power"][0] > 0) == (psy in (1, 3)) and (per["bark"][0] > 0) == (psy in (1, 3))
    assert (per["cand"][0] > 0) == (psy == 1) and (per["xmax"][0] > 0) == (psy == 3)
    if psy in (1, 3):
        nch = 1 if mode == "m" else 2
        assert per["power"][0] >= 512 * nch * units                  # every line's energy meets the floor once (the near-1 lines twice)
        assert per["smr"][0] == 32 * nch * units
