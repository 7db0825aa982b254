"""The true-peak limiter's C-ABI without a GPU: the header declares exactly the tlb_*limiter* names and the library exports each, none of
them claimed by another ABI test's word, the record is 32 bytes with the field offsets of the binding's dtype (a translation unit compiled
against the header says so), tlb_limiter_step computes, and the NULL-handle calls answer without touching a device."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_limiter_enable", "tlb_limiter_device", "tlb_limiter_host", "tlb_limiter_reset", "tlb_limiter_step",
         "tlb_tick_enable_limiter", "tlb_tick_limiter", "tlb_tick_limiter_reset",
         "tlb_node_enable_limiter", "tlb_node_limiter", "tlb_node_limiter_reset"]
OTHERS = ("monitor", "compare", "feed", "resample", "decimate", "decode", "loudness", "truepeak")      # words whose own ABI tests claim every name that contains them
RATES = (48000, 44100, 32000, 24000, 22050, 16000)


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_exactly_the_names(M):
    src = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*limiter[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {n for n in exported if "limiter" in n} == set(NAMES)
    assert not [n for n in NAMES for w in OTHERS if w in n]
    for name, value in (("TLB_LIMITER_WMIN", "64"), ("TLB_LIMITER_WBOX", "32"), ("TLB_LIMITER_DELAY", "63"), ("TLB_LIMITER_RELEASE_DEFAULT_MS", "100u")):
        assert re.search(r"#define %s %s\b" % (name, value), src), name
    assert M.LIMITER_DELAY == 63


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_record_is_32_bytes_with_the_offsets_of_the_dtype(M, tmp_path):
    ctype, dt = "tlb_limiter_record", M.LIMITER_DTYPE
    fields = list(dt.names)
    assert fields == ["frames", "limited", "samples", "red_last", "red_max", "peak_in", "peak_in_max", "reserved"]
    prog = tmp_path / (ctype + ".c")
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "toolame_batch.h"\nint main(void) {\n    printf("%%zu %%zu", sizeof(%s), sizeof(tlb_limiter_params));\n' % ctype
                    + "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields)
                    + '    printf(" %zu %zu", offsetof(tlb_limiter_params, ceiling), offsetof(tlb_limiter_params, release_ms));\n    return 0;\n}\n')
    exe = tmp_path / ctype
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 32 == dt.itemsize and got[1] == 8
    assert got[2:10] == [dt.fields[f][1] for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert got[10:] == [0, 4]
    import limiterlib as LM
    assert LM.RECORD.itemsize == 32 and [LM.RECORD.fields[f][1] for f in LM.RECORD.names] == got[2:10] and list(LM.RECORD.names) == fields


def test_limiter_step_for_the_six_rates(M):
    """S = max(1, (2^30 * 1000) / (release_ms * samplerate)) in integers, at 1, 100 and 10000 ms; 0 ms is the default 100"""
    for rate in RATES:
        for ms in (1, 100, 10000):
            want = max(1, (2 ** 30 * 1000) // (ms * rate))
            assert M.limiter_step(ms, rate) == want, (ms, rate)
            assert 1 <= want <= 2 ** 26
        assert M.limiter_step(0, rate) == M.limiter_step(100, rate)
    assert M.limiter_step(1, 16000) == 2 ** 26 and M.limiter_step(100, 48000) == 223696 and M.limiter_step(10000, 48000) == 2236
    assert M.limiter_step(10001, 48000) == 0 and M.limiter_step(100, 0) == 0 and M.limiter_step(100, -48000) == 0
    import limiterlib as LM
    assert all(LM.step(ms, rate) == M.limiter_step(ms, rate) for rate in RATES for ms in (0, 1, 7, 100, 10000))


def test_null_handles_answer_without_a_gpu(M):
    L = M.load_library()
    ARG = 18
    rec = np.zeros(4, dtype=M.LIMITER_DTYPE)
    pcm = np.zeros((1, 4, 2, 1152), dtype=np.int16)
    params = (np.zeros(2, dtype=np.uint32)).ctypes.data
    assert L.tlb_limiter_enable(None, params) == ARG and L.tlb_limiter_enable(None, None) == ARG and L.tlb_limiter_reset(None, -1) == ARG
    assert L.tlb_limiter_device(None, pcm.ctypes.data, 1, rec.ctypes.data, None) == ARG
    assert L.tlb_limiter_host(None, pcm.ctypes.data, 1, rec.ctypes.data) == ARG
    assert L.tlb_tick_enable_limiter(None, params) == ARG and L.tlb_tick_limiter_reset(None, 0) == ARG
    assert L.tlb_node_enable_limiter(None, params) == ARG and L.tlb_node_limiter_reset(None, -1) == ARG
    assert L.tlb_tick_limiter(None) is None and L.tlb_node_limiter(None, 0) is None
    assert not rec.view(np.uint8).any() and not pcm.any()
