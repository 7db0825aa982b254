"""The compare monitor's C-ABI without a GPU: the header declares every tlb_*compare* name and the library exports each, none of the new
names contains `monitor` (tests/test_monitor_abi.py pins that set), the record is 96 bytes with the field offsets of COMPARE_DTYPE (a
translation unit compiled against the header says so), and the NULL-handle calls answer without touching a device."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_compare_device", "tlb_compare_host", "tlb_compare_reset", "tlb_tick_enable_compare", "tlb_tick_compare", "tlb_node_enable_compare",
         "tlb_node_compare"]
MONITOR_NAMES = ["tlb_monitor_device", "tlb_monitor_host", "tlb_tick_enable_monitor", "tlb_tick_monitor", "tlb_tick_monitor_listen", "tlb_tick_monitor_pcm",
                 "tlb_node_enable_monitor", "tlb_node_monitor", "tlb_node_monitor_listen", "tlb_node_monitor_pcm"]


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_every_name(M):
    src = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*compare[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {n for n in exported if "compare" in n} == set(NAMES)
    assert not [n for n in NAMES if "monitor" in n] and {n for n in exported if "monitor" in n} == set(MONITOR_NAMES)
    for name, value in (("TLB_COMPARE_DELAY", "481"), ("TLB_COMPARE_JUDGED0", "0x01u"), ("TLB_COMPARE_JUDGED1", "0x02u"), ("TLB_COMPARE_MISMATCH", "0x04u"),
                        ("TLB_COMPARE_SWAPPED", "0x08u"), ("TLB_COMPARE_SKIPPED", "0x10u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), src), name
    d = {k: int(re.search(r"#define\s+TLB_COMPARE_DEFAULT_%s\s+(\d+)" % k, src).group(1)) for k in ("MIN_ENERGY", "CORR_NUM", "CORR_DEN")}
    assert (d["MIN_ENERGY"], d["CORR_NUM"], d["CORR_DEN"]) == M.COMPARE_DEFAULTS and 0 < d["CORR_NUM"] <= d["CORR_DEN"] <= 1024 and d["MIN_ENERGY"] >= 1
    assert (M.COMPARE_JUDGED0, M.COMPARE_JUDGED1, M.COMPARE_MISMATCH, M.COMPARE_SWAPPED, M.COMPARE_SKIPPED) == (1, 2, 4, 8, 16)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_record_is_96_bytes_with_the_offsets_of_the_dtype(M, tmp_path):
    fields = list(M.COMPARE_DTYPE.names)
    pfields = list(M.COMPARE_PARAMS_DTYPE.names)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "toolame_batch.h"\nint main(void) {\n    printf("%zu", sizeof(tlb_compare_record));\n'
                    + "".join('    printf(" %%zu", offsetof(tlb_compare_record, %s));\n' % f for f in fields)
                    + '    printf(" %zu", sizeof(tlb_compare_params));\n'
                    + "".join('    printf(" %%zu", offsetof(tlb_compare_params, %s));\n' % f for f in pfields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert got[0] == 96 == M.COMPARE_DTYPE.itemsize
    assert got[1:1 + n] == [M.COMPARE_DTYPE.fields[f][1] for f in fields] == [0, 16, 32, 48, 64, 68, 72, 76, 80, 84, 88]
    assert got[1 + n] == 16 == M.COMPARE_PARAMS_DTYPE.itemsize and got[2 + n:] == [M.COMPARE_PARAMS_DTYPE.fields[f][1] for f in pfields] == [0, 8, 12]
    for k in ("sxx", "syy", "sxy", "sxz"):
        assert M.COMPARE_DTYPE[k].shape == (2,) and M.COMPARE_DTYPE[k].base == np.int64
    import comparelib as CL
    assert CL.RECORD_DTYPE == M.COMPARE_DTYPE


def test_null_handles_answer_without_a_gpu(M):
    L = M.load_library()
    ARG = 18
    rec = np.zeros(4, dtype=M.COMPARE_DTYPE)
    rep = np.zeros((1, 4), dtype=M.FRAME_REPORT_DTYPE)
    pcm = np.zeros((1, 4, 2, 1152), dtype=np.int16)
    par = M.compare_params((1152 * 256 * 256, 1, 2))
    assert L.tlb_compare_device(None, pcm.ctypes.data, pcm.ctypes.data, rep.ctypes.data, 1, par.ctypes.data, rec.ctypes.data, None) == ARG
    assert L.tlb_compare_host(None, pcm.ctypes.data, pcm.ctypes.data, rep.ctypes.data, 1, par.ctypes.data, rec.ctypes.data) == ARG
    assert L.tlb_compare_reset(None, -1) == ARG and L.tlb_compare_reset(None, 0) == ARG
    assert not rec.view(np.uint8).any()
    assert L.tlb_tick_enable_compare(None, par.ctypes.data) == ARG and L.tlb_node_enable_compare(None, par.ctypes.data) == ARG
    assert L.tlb_tick_enable_compare(None, None) == ARG and L.tlb_node_enable_compare(None, None) == ARG
    assert L.tlb_tick_compare(None) is None and L.tlb_node_compare(None, 0) is None
    # the monitor's `what` values are what they were: 3 and 4 are no modes
    assert L.tlb_tick_enable_monitor(None, 3) == ARG and L.tlb_tick_enable_monitor(None, 4) == ARG
