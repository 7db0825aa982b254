"""The loudness meter's C-ABI without a GPU: the header declares exactly the tlb_*loudness* names and the library exports each, the records
are 48 and 24 bytes with the field offsets of the binding's dtypes (a translation unit compiled against the header says so), and the
NULL-handle calls answer without touching a device."""
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_loudness_enable", "tlb_loudness_device", "tlb_loudness_host", "tlb_loudness_programme_device", "tlb_loudness_programme_host",
         "tlb_loudness_reset", "tlb_loudness_taps", "tlb_loudness_scale", "tlb_loudness_lufs",
         "tlb_tick_enable_loudness", "tlb_tick_loudness", "tlb_tick_loudness_programme", "tlb_tick_loudness_reset",
         "tlb_node_enable_loudness", "tlb_node_loudness", "tlb_node_loudness_programme", "tlb_node_loudness_reset"]
OTHERS = ("monitor", "compare", "feed", "resample", "decimate", "decode")      # words whose own ABI tests claim every name that contains them


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_exactly_the_names(M):
    src = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*loudness[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {n for n in exported if "loudness" in n} == set(NAMES)
    assert not [n for n in NAMES for w in OTHERS if w in n]
    assert re.search(r"#define\s+TLB_LOUDNESS_BINS\s+751\b", src)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_records_are_48_and_24_bytes_with_the_offsets_of_the_dtypes(M, tmp_path):
    for ctype, dt, size, offs in (("tlb_loudness_record", M.LOUDNESS_DTYPE, 48, [0, 4, 8, 12, 16, 24, 32, 40]),
                                  ("tlb_loudness_programme_record", M.LOUDNESS_PROGRAMME_DTYPE, 24, [0, 8, 16, 20])):
        fields = list(dt.names)
        prog = tmp_path / (ctype + ".c")
        prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "toolame_batch.h"\nint main(void) {\n    printf("%%zu", sizeof(%s));\n' % ctype
                        + "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) + "    return 0;\n}\n")
        exe = tmp_path / ctype
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(prog)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got[0] == size == dt.itemsize
        assert got[1:] == [dt.fields[f][1] for f in fields] == offs


def test_null_handles_answer_without_a_gpu(M):
    L = M.load_library()
    ARG = 18
    rec = np.zeros(4, dtype=M.LOUDNESS_DTYPE)
    prog = np.zeros(4, dtype=M.LOUDNESS_PROGRAMME_DTYPE)
    pcm = np.zeros((1, 4, 2, 1152), dtype=np.int16)
    assert L.tlb_loudness_enable(None) == ARG and L.tlb_loudness_reset(None, -1) == ARG
    assert L.tlb_loudness_device(None, pcm.ctypes.data, 1, rec.ctypes.data, None) == ARG
    assert L.tlb_loudness_host(None, pcm.ctypes.data, 1, rec.ctypes.data) == ARG
    assert L.tlb_loudness_programme_device(None, prog.ctypes.data, None) == ARG and L.tlb_loudness_programme_host(None, prog.ctypes.data) == ARG
    assert L.tlb_tick_enable_loudness(None) == ARG and L.tlb_tick_loudness_programme(None, prog.ctypes.data) == ARG and L.tlb_tick_loudness_reset(None, 0) == ARG
    assert L.tlb_node_enable_loudness(None) == ARG and L.tlb_node_loudness_programme(None, prog.ctypes.data) == ARG and L.tlb_node_loudness_reset(None, -1) == ARG
    assert L.tlb_tick_loudness(None) is None and L.tlb_node_loudness(None, 0) is None
    assert not rec.view(np.uint8).any() and not prog.view(np.uint8).any()
    assert L.tlb_loudness_taps(48000, None) == ARG and L.tlb_loudness_taps(12345, np.zeros(10).ctypes.data) == 1
    assert M.loudness_lufs(0.0) == -math.inf and M.loudness_lufs(1.0) == -0.691 and abs(M.loudness_lufs(10.0 ** -2.2309) - (-23.0)) < 1e-9
