"""Support for the confidence monitor tests (test_monitor_emu.py, test_monitor_gpu.py): the emulation of the fold kernel
(tests/emu/mp2_monitor_emu.cpp, compiled into a temporary directory) and the rule of include/toolame_batch.h (tlb_monitor_device) as a
plain Python loop -- the fold's oracle."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from declib import BAD_MASK, EMPTY, REPORT_DTYPE
from ingestlib import FS_IDX, frame_ms

ROOT = Path(__file__).resolve().parent.parent
RECORD_DTYPE = np.dtype([("frames", np.uint32), ("bad_frames", np.uint32), ("bad_run", np.uint32), ("flags_seen", np.uint32),
                         ("last_status", np.uint32), ("out_silence_ms", np.uint32), ("out_peak", np.int16, (2,)), ("reserved_", np.uint32)])
FIELDS = ("frames", "bad_frames", "bad_run", "flags_seen", "last_status", "out_silence_ms", "reserved_")


def build_emu(outdir):
    """tests/emu/mp2_monitor_emu.cpp -> outdir/libmp2monitoremu.so (the flags of tests/emu/Makefile)"""
    so = Path(outdir) / "libmp2monitoremu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function",
                    "-Wno-unused-variable", "-Wno-unknown-pragmas", "-shared", "-o", str(so), str(ROOT / "tests" / "emu" / "mp2_monitor_emu.cpp"), "-lm"], check=True)
    return so


class MonitorEmu:
    def __init__(self, so):
        L = self.L = C.CDLL(str(so))
        L.mon_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.mon_sizeof_record() == RECORD_DTYPE.itemsize == 32

    def fold(self, report, pcm, rates, nch, record):
        """one call over report [nf][ns] (and pcm [nf][ns][2][1152] or None); record RECORD_DTYPE [ns] is advanced in place"""
        rep = np.ascontiguousarray(report, dtype=REPORT_DTYPE)
        nf, ns = rep.shape
        pc = None if pcm is None else np.ascontiguousarray(pcm, dtype=np.int16)
        assert pc is None or pc.shape == (nf, ns, 2, 1152)
        ver = np.array([FS_IDX[r][0] for r in rates], dtype=np.int32)
        fsi = np.array([FS_IDX[r][1] for r in rates], dtype=np.int32)
        nc = np.ascontiguousarray(nch, dtype=np.int32)
        assert record.dtype == RECORD_DTYPE and record.shape == (ns,) and record.flags.c_contiguous
        rc = self.L.mon_fold(rep.ctypes.data, None if pc is None else pc.ctypes.data, nf, ns, ver.ctypes.data, fsi.ctypes.data, nc.ctypes.data, record.ctypes.data)
        assert rc == 0, rc


def fold_python(status, pcm, rates, record=None):
    """The rule, slot by slot.  status [nf][ns] (ints), pcm [nf][ns][2][1152] or None, rates [ns] in Hz; record: a RECORD_DTYPE [ns] to go
    on from (not changed) or None for zeros -> a new RECORD_DTYPE [ns]"""
    status = np.asarray(status)
    nf, ns = status.shape
    out = np.zeros(ns, dtype=RECORD_DTYPE) if record is None else record.copy()
    for s in range(ns):
        r = {k: int(out[s][k]) for k in FIELDS}
        peak = [int(out[s]["out_peak"][0]), int(out[s]["out_peak"][1])]
        for f in range(nf):
            st = int(status[f, s])
            r["last_status"] = st
            r["flags_seen"] |= st
            if st & EMPTY:
                peak = [0, 0]
                continue
            r["frames"] += 1
            if st & BAD_MASK:
                r["bad_frames"] += 1
                r["bad_run"] += 1
            else:
                r["bad_run"] = 0
            if pcm is not None:
                peak = [max(0, int(pcm[f, s, c].max())) for c in range(2)]
                r["out_silence_ms"] = r["out_silence_ms"] + frame_ms(rates[s]) if peak == [0, 0] else 0
        for k in FIELDS:
            out[s][k] = r[k]
        out[s]["out_peak"] = peak
    return out


def reports_of(status):
    """status ints [nf][ns] -> REPORT_DTYPE [nf][ns] with the other fields filled with values the fold must not look at"""
    status = np.asarray(status, dtype=np.uint32)
    rep = np.zeros(status.shape, dtype=REPORT_DTYPE)
    rep["status"] = status
    rep["crc_stored"] = 0xbeef
    rep["crc_computed"] = 0x1234
    rep["mode"] = 3
    rep["mode_ext"] = 2
    rep["audio_bits"] = 0xffff
    return rep
