"""The confidence monitor's C-ABI without a GPU: the header declares every tlb_*monitor* name and the library exports each, the record is
32 bytes with the field offsets of MONITOR_DTYPE (a translation unit compiled against the header says so), and the NULL-handle calls
answer without touching a device."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_monitor_device", "tlb_monitor_host", "tlb_tick_enable_monitor", "tlb_tick_monitor", "tlb_tick_monitor_listen", "tlb_tick_monitor_pcm",
         "tlb_node_enable_monitor", "tlb_node_monitor", "tlb_node_monitor_listen", "tlb_node_monitor_pcm"]


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_every_name(M):
    src = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*monitor[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NAMES) <= exported
    assert {n for n in exported if "monitor" in n} == set(NAMES)
    for name, value in (("TLB_MONITOR_CHECK", 1), ("TLB_MONITOR_AUDIO", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), src)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_record_is_32_bytes_with_the_offsets_of_the_dtype(M, tmp_path):
    from odr_audioenc_amd.toolame import MONITOR_DTYPE
    assert MONITOR_DTYPE.itemsize == 32
    fields = list(MONITOR_DTYPE.names)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "toolame_batch.h"\nint main(void) {\n    printf("%zu", sizeof(tlb_monitor_record));\n'
                    + "".join('    printf(" %%zu", offsetof(tlb_monitor_record, %s));\n' % f for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 32
    assert got[1:] == [MONITOR_DTYPE.fields[f][1] for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert MONITOR_DTYPE["out_peak"].shape == (2,) and MONITOR_DTYPE["out_peak"].base == np.int16


def test_null_handles_answer_without_a_gpu(M):
    L = M.load_library()
    ARG = 18
    rec = np.zeros(4, dtype=M.MONITOR_DTYPE)
    rep = np.zeros((1, 4), dtype=M.FRAME_REPORT_DTYPE)
    assert L.tlb_monitor_device(None, rep.ctypes.data, None, 1, rec.ctypes.data, None) == ARG
    assert L.tlb_monitor_host(None, rep.ctypes.data, None, 1, rec.ctypes.data) == ARG
    assert not rec.view(np.uint8).any()
    assert L.tlb_tick_enable_monitor(None, 1) == ARG and L.tlb_tick_enable_monitor(None, 2) == ARG
    assert L.tlb_tick_monitor_listen(None, 0) == ARG and L.tlb_tick_monitor_listen(None, -1) == ARG
    assert L.tlb_node_enable_monitor(None, 2) == ARG and L.tlb_node_monitor_listen(None, 0) == ARG
    assert L.tlb_tick_monitor(None) is None and L.tlb_node_monitor(None, 0) is None
    s = C.c_int(7)
    assert L.tlb_tick_monitor_pcm(None, C.byref(s)) is None and s.value == -1
    s = C.c_int(7)
    assert L.tlb_node_monitor_pcm(None, C.byref(s)) is None and s.value == -1
    assert L.tlb_tick_monitor_pcm(None, None) is None and L.tlb_node_monitor_pcm(None, None) is None
