"""The true-peak meter's C-ABI without a GPU: the header declares exactly the tlb_*truepeak* names and the library exports each, the record
is 32 bytes with the field offsets of the binding's dtype (a translation unit compiled against the header says so), the no-GPU helpers
compute, and the NULL-handle calls answer without touching a device."""
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_truepeak_enable", "tlb_truepeak_device", "tlb_truepeak_host", "tlb_truepeak_reset", "tlb_truepeak_taps", "tlb_truepeak_dbtp",
         "tlb_tick_enable_truepeak", "tlb_tick_truepeak", "tlb_tick_truepeak_reset",
         "tlb_node_enable_truepeak", "tlb_node_truepeak", "tlb_node_truepeak_reset"]
OTHERS = ("monitor", "compare", "feed", "resample", "decimate", "decode", "loudness")      # words whose own ABI tests claim every name that contains them


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_exactly_the_names(M):
    src = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*truepeak[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {n for n in exported if "truepeak" in n} == set(NAMES)
    assert not [n for n in NAMES for w in OTHERS if w in n]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_record_is_32_bytes_with_the_offsets_of_the_dtype(M, tmp_path):
    ctype, dt = "tlb_truepeak_record", M.TRUEPEAK_DTYPE
    fields = list(dt.names)
    assert fields == ["frames", "overs", "peak", "peak_max", "sample_max"]
    prog = tmp_path / (ctype + ".c")
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "toolame_batch.h"\nint main(void) {\n    printf("%%zu", sizeof(%s));\n' % ctype
                    + "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / ctype
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 32 == dt.itemsize
    assert got[1:] == [dt.fields[f][1] for f in fields] == [0, 4, 8, 16, 24]
    assert dt["peak"].shape == dt["peak_max"].shape == dt["sample_max"].shape == (2,)


def test_helpers_compute_without_a_gpu(M):
    assert M.truepeak_dbtp(2 ** 30) == 0.0 and M.truepeak_dbtp(0) == -math.inf
    assert abs(M.truepeak_dbtp(M.TRUEPEAK_CEILING_DEFAULT) - (-1.0)) < 1e-8
    assert abs(M.truepeak_dbtp(2 ** 29) - 20.0 * math.log10(0.5)) < 1e-12
    assert M.truepeak_dbtp(2 ** 32 - 1) > 12.0                       # the whole unsigned range is taken as unsigned
    assert M.truepeak_taps().shape == (3, 12)


def test_null_handles_answer_without_a_gpu(M):
    L = M.load_library()
    ARG = 18
    rec = np.zeros(4, dtype=M.TRUEPEAK_DTYPE)
    pcm = np.zeros((1, 4, 2, 1152), dtype=np.int16)
    assert L.tlb_truepeak_enable(None, 0) == ARG and L.tlb_truepeak_reset(None, -1) == ARG
    assert L.tlb_truepeak_device(None, pcm.ctypes.data, 1, rec.ctypes.data, None) == ARG
    assert L.tlb_truepeak_host(None, pcm.ctypes.data, 1, rec.ctypes.data) == ARG
    assert L.tlb_tick_enable_truepeak(None, 0) == ARG and L.tlb_tick_truepeak_reset(None, 0) == ARG
    assert L.tlb_node_enable_truepeak(None, 0) == ARG and L.tlb_node_truepeak_reset(None, -1) == ARG
    assert L.tlb_tick_truepeak(None) is None and L.tlb_node_truepeak(None, 0) is None
    assert not rec.view(np.uint8).any()
