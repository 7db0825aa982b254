"""Support for the short-read tests (test_short_reads_emu.py, test_short_reads_gpu.py): the emulation of the kernels of the caller's glue
(tests/emu/mp2_ingest_emu.cpp, compiled into a temporary directory), a numpy statement of the three cases of include/toolame_batch.h
(tlb_ingest_device_valid) and the two counters as plain loops."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FRAMES = 1152
FS_IDX = {44100: (1, 0), 48000: (1, 1), 32000: (1, 2), 22050: (0, 0), 24000: (0, 1), 16000: (0, 2)}      # rate -> (MPEG version bit, sampling_frequency index)


def build_emu(outdir):
    """tests/emu/mp2_ingest_emu.cpp -> outdir/libmp2ingestemu.so (the flags of tests/emu/Makefile)"""
    so = Path(outdir) / "libmp2ingestemu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function",
                    "-Wno-unused-variable", "-Wno-unknown-pragmas", "-shared", "-o", str(so), str(ROOT / "tests" / "emu" / "mp2_ingest_emu.cpp"), "-lm"], check=True)
    return so


def gain_of(db):
    """tlb_set_gain_db: pow(10.0, gain_db / 20.0) (src/odr-audioenc.cpp:1032)"""
    return math.pow(10.0, db / 20.0)


class IngestEmu:
    def __init__(self, so):
        L = self.L = C.CDLL(str(so))
        L.ing_ingest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ing_underrun.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ing_silence.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ing_src.argtypes = [C.c_int, C.c_int]

    def ingest(self, inter, valid, nch, gains_db):
        """inter [nf][ns][2304] int16, valid [nf][ns] or None -> (pcm [nf][ns][2][1152], peaks [nf][ns][2])"""
        inter = np.ascontiguousarray(inter, dtype=np.int16)
        nf, ns = inter.shape[:2]
        assert inter.shape == (nf, ns, 2 * FRAMES)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.int32)
        assert v is None or v.shape == (nf, ns)
        nc = np.ascontiguousarray(nch, dtype=np.int32)
        g = np.array([gain_of(x) for x in gains_db], dtype=np.float64)
        assert nc.shape == (ns,) and g.shape == (ns,)
        out = np.full((nf, ns, 2, FRAMES), 0x5555, dtype=np.int16)     # every value must be written
        pk = np.full((nf, ns, 2), 0x5555, dtype=np.int16)
        rc = self.L.ing_ingest(inter.ctypes.data, None if v is None else v.ctypes.data, nf, ns, nc.ctypes.data, g.ctypes.data, out.ctypes.data, pk.ctypes.data)
        assert rc == 0, rc
        return out, pk

    def underrun(self, valid, rates, nch, underrun_ms, underruns):
        """one call over valid [nf][ns]; the two uint32 [ns] arrays are updated in place"""
        v = np.ascontiguousarray(valid, dtype=np.int32)
        nf, ns = v.shape
        ver = np.array([FS_IDX[r][0] for r in rates], dtype=np.int32)
        fsi = np.array([FS_IDX[r][1] for r in rates], dtype=np.int32)
        nc = np.ascontiguousarray(nch, dtype=np.int32)
        assert underrun_ms.dtype == np.uint32 and underruns.dtype == np.uint32 and underrun_ms.shape == (ns,) and underruns.shape == (ns,)
        rc = self.L.ing_underrun(v.ctypes.data, nf, ns, ver.ctypes.data, fsi.ctypes.data, nc.ctypes.data, underrun_ms.ctypes.data, underruns.ctypes.data)
        assert rc == 0, rc

    def silence(self, peaks, rates, nch, silence_ms):
        """one call over peaks [nf][ns][2] int16; the uint32 [ns] array is updated in place"""
        pk = np.ascontiguousarray(peaks, dtype=np.int16)
        nf, ns = pk.shape[:2]
        assert pk.shape == (nf, ns, 2) and silence_ms.dtype == np.uint32 and silence_ms.shape == (ns,)
        ver = np.array([FS_IDX[r][0] for r in rates], dtype=np.int32)
        fsi = np.array([FS_IDX[r][1] for r in rates], dtype=np.int32)
        nc = np.ascontiguousarray(nch, dtype=np.int32)
        rc = self.L.ing_silence(pk.ctypes.data, nf, ns, ver.ctypes.data, fsi.ctypes.data, nc.ctypes.data, silence_ms.ctypes.data)
        assert rc == 0, rc


# ---------------------------------------------------------------------------------------------------------------------------------
# the three cases in numpy (include/toolame_batch.h, tlb_ingest_device_valid)
def src_index(valid):
    """-> (src [1152] source frame of every output frame, live [1152] False where the output is a zero of the tail)"""
    v = min(max(int(valid), 0), FRAMES)
    missing = FRAMES - v
    i = np.arange(FRAMES)
    if missing == 0 or missing >= 116:
        src = i
    else:
        q = v // missing
        src = np.where(i >= 1, i - (i - 1) // q, 0)
    return src, src < v


def stretch(slot, valid, nch):
    """slot [2304] int16 as the caller holds it (junk behind valid) -> the stretched interleaved buffer [2304] (mono: its first 1152)"""
    src, live = src_index(valid)
    out = slot.copy()
    if nch == 2:
        fr = slot.reshape(FRAMES, 2)
        out[:] = np.where(live[:, None], fr[np.minimum(src, FRAMES - 1)], 0).reshape(-1)
    else:
        out[:FRAMES] = np.where(live, slot[np.minimum(src, FRAMES - 1)], 0)
    return out


def stretch_batch(inter, valid, nch):
    out = inter.copy()
    for f in range(inter.shape[0]):
        for s in range(inter.shape[1]):
            out[f, s] = stretch(inter[f, s], valid[f, s], nch[s])
    return out


def ingest_numpy(inter, valid, nch, gains_db):
    """stretch, then gain with the double-multiply-and-truncate, the positive peaks of the values at even / odd positions, the de-interleave"""
    nf, ns = inter.shape[:2]
    st = stretch_batch(inter, valid, nch)
    out = np.zeros((nf, ns, 2, FRAMES), dtype=np.int16)
    pk = np.zeros((nf, ns, 2), dtype=np.int16)
    for s in range(ns):
        n = 2 * FRAMES if nch[s] == 2 else FRAMES
        g = gain_of(gains_db[s])
        x = st[:, s, :n]
        if g != 1.0:
            x = np.trunc(x.astype(np.float64) * g).astype(np.int64).astype(np.int16)        # (short)(int)(x * g)
        pk[:, s, 0] = np.maximum(x[:, 0::2].max(axis=1), 0)
        pk[:, s, 1] = np.maximum(x[:, 1::2].max(axis=1), 0)
        if nch[s] == 2:
            out[:, s, 0] = x[:, 0::2]
            out[:, s, 1] = x[:, 1::2]
        else:
            out[:, s, 0] = x
    return out, pk


def frame_ms(rate):
    """whole milliseconds of a frame as the reference's silence counter computes them (src/odr-audioenc.cpp:1053-1062)"""
    return 1000 * 1152 // rate


def underrun_python(valid, rates, ms0, n0):
    ms, n = [int(x) for x in ms0], [int(x) for x in n0]
    for f in range(valid.shape[0]):
        for s in range(valid.shape[1]):
            if valid[f, s] < FRAMES:
                ms[s] += frame_ms(rates[s]); n[s] += 1
            else:
                ms[s] = 0
    return ms, n


def silence_python(peaks, rates, ms0):
    """a frame whose peaks are both 0 adds its whole milliseconds, any other frame resets the counter (src/odr-audioenc.cpp:1053-1079)"""
    ms = [int(x) for x in ms0]
    for f in range(peaks.shape[0]):
        for s in range(peaks.shape[1]):
            ms[s] = ms[s] + frame_ms(rates[s]) if max(int(peaks[f, s, 0]), int(peaks[f, s, 1])) == 0 else 0
    return ms


# the batch of the silence tests (test_short_reads_emu.py, test_hip_parity.py): every rate with two channels and with one, 16 frames fed in
# these cuts, counters that do not start at 0.  Streams in fours, by column: always silent; never silent; silent but for the last frame;
# silent but for peaks (0, 3) once in the middle
SILENCE_RATES = [48000, 32000, 24000, 16000, 44100, 22050]
SILENCE_CUTS = (1, 7, 3, 2, 1, 2)


def silence_case():
    """-> (rates [12], nch [12], peaks [16][12][2] int16, start [12] uint32)"""
    rates = SILENCE_RATES + SILENCE_RATES
    nch = [2] * 6 + [1] * 6
    nf, ns = sum(SILENCE_CUTS), len(rates)
    rng = np.random.default_rng(1053)
    peaks = np.zeros((nf, ns, 2), dtype=np.int16)
    for s in range(ns):
        col = s % 4
        if col == 1:
            peaks[:, s] = rng.integers(1, 32768, size=(nf, 2))
        elif col == 2:
            peaks[-1, s] = (int(rng.integers(1, 32768)), 0)
        elif col == 3:
            peaks[nf // 2, s] = (0, 3)
    start = (1000 + 7 * np.arange(ns)).astype(np.uint32)
    return rates, nch, peaks, start


def fixture():
    z = np.load(GOLDEN / "short_reads.npz")
    return z["valid"], z["stereo"], z["mono"]
