"""The loudness range's C-ABI without a GPU: the header declares exactly the tlb_*lra* names and the library exports each, the record is 40
bytes with the field offsets of the binding's dtype (a translation unit compiled against the header says so), the NULL-handle calls answer
without touching a device, and tlb_lra_lu is 0.1 * (high_bin - low_bin)."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_lra_enable", "tlb_lra_device", "tlb_lra_host", "tlb_lra_lu", "tlb_tick_enable_lra", "tlb_tick_lra", "tlb_node_enable_lra", "tlb_node_lra"]
# words whose own ABI tests claim every name that contains them
OTHERS = ("loudness", "monitor", "compare", "feed", "resample", "decimate", "decode", "conceal", "truepeak", "limiter")


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_exactly_the_names(M):
    src = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*lra[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {n for n in exported if re.search(r"(^|_)lra(_|$)", n)} == set(NAMES)
    assert not [n for n in NAMES for w in OTHERS if w in n]
    assert "loudness range (LRA)" not in HEADER.read_text()          # no longer listed as not built


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_record_is_40_bytes_with_the_offsets_of_the_dtype(M, tmp_path):
    ctype, dt, size, offs = "tlb_lra_record", M.LRA_DTYPE, 40, [0, 8, 16, 24, 28, 32, 36]
    fields = list(dt.names)
    assert fields == ["low", "high", "gate", "blocks", "gated", "low_bin", "high_bin"]
    prog = tmp_path / (ctype + ".c")
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "toolame_batch.h"\nint main(void) {\n    printf("%%zu", sizeof(%s));\n' % ctype
                    + "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / ctype
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == size == dt.itemsize
    assert got[1:] == [dt.fields[f][1] for f in fields] == offs
    assert [dt.fields[f][0].str for f in fields] == ["<f8", "<f8", "<f8", "<u4", "<u4", "<i4", "<i4"]


def test_null_handles_answer_without_a_gpu(M):
    L = M.load_library()
    ARG = 18
    rec = np.zeros(4, dtype=M.LRA_DTYPE)
    assert L.tlb_lra_enable(None) == ARG
    assert L.tlb_lra_device(None, rec.ctypes.data, None) == ARG and L.tlb_lra_host(None, rec.ctypes.data) == ARG
    assert L.tlb_tick_enable_lra(None) == ARG and L.tlb_tick_lra(None, rec.ctypes.data) == ARG
    assert L.tlb_node_enable_lra(None) == ARG and L.tlb_node_lra(None, rec.ctypes.data) == ARG
    assert not rec.view(np.uint8).any()


def test_lra_lu(M):
    L = M.load_library()
    assert L.tlb_lra_lu(None) == 0.0
    rec = np.zeros((), dtype=M.LRA_DTYPE)
    assert M.lra_lu(rec) == 0.0
    for lo, hi in ((350, 500), (0, 750), (417, 417), (300, 301), (123, 456)):
        rec["low_bin"], rec["high_bin"] = lo, hi
        assert M.lra_lu(rec) == 0.1 * (hi - lo)
    rec["low_bin"], rec["high_bin"] = 350, 500
    assert M.lra_lu(rec) == 15.0
    raw = (C.c_uint8 * 40)()
    assert L.tlb_lra_lu(C.addressof(raw)) == 0.0
