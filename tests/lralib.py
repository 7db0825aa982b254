"""Support for the loudness range tests (test_lra_*.py): the definition of include/toolame_batch.h ("Loudness range", tlb_lra_*) restated --
the oracle, nothing else: the range rule on Python ints and numpy float64 (range_rule), the range blocks from the short-term values that
loudnesslib.Oracle forms (Oracle), no code shared with the emulation -- the emulation of the kernels (tests/emu/mp2_lra_emu.cpp, compiled
into a temporary directory on first use, and the same text behind tests/emu/lra_sanitize_main.cpp with AddressSanitizer + UBSan), and the
stream sets and signals the test files share."""
import ctypes as C
import math

import numpy as np

import loudnesslib as LL

N = LL.N
NBINS = LL.NBINS
HIST_ROWS = LL.HIST_ROWS
RECORD = np.dtype([("low", "<f8"), ("high", "<f8"), ("gate", "<f8"), ("blocks", "<u4"), ("gated", "<u4"), ("low_bin", "<i4"), ("high_bin", "<i4")])
# the device test's shape: 37 streams = 74 lanes, a full wave and a second one with five streams; 230 frames = 264 960 samples: 55 bins and
# 26 range blocks at 48 kHz ... 165 bins and 136 range blocks at 16 kHz
STREAMS = LL.STREAMS
NFRAMES = 230
CUTS = ((230,), (1,) * 230, (7, 223))
SILENT, QUIET, CONSTANT = 5, 11, 17                                  # streams of the set with a signal of their own (signal())
# the oracle's shape (its Python loop runs over every sample): every rate with one and with two channels and a thirteenth stream; 140
# frames = 161 280 samples: 33 bins and 4 range blocks at 48 kHz ... 100 bins and 71 range blocks at 16 kHz
ORACLE_STREAMS = [dict(samplerate=LL.RATES[s % 6], mode="m" if (s // 6 + s) % 2 else "s") for s in range(13)]
ORACLE_NFRAMES = 140
ORACLE_CUTS = ((140,), (1,) * 140, (7, 133), (64, 13, 63))


def range_rule(counts, centres):
    """751 counts (any integers) -> (low, high, gate, N, N2, low_bin, high_bin): the header's rule, the counts as Python ints"""
    n = [int(v) for v in counts]
    assert len(n) == NBINS
    total = sum(n)
    if not total:
        return (0.0, 0.0, 0.0, 0, 0, 0, 0)
    S = np.float64(0.0)
    for j in range(NBINS):
        S = S + np.float64(n[j]) * centres[j]
    gate = np.float64(0.01) * (S / np.float64(total))
    gated = [j for j in range(NBINS) if centres[j] >= gate]
    n2 = sum(n[j] for j in gated)
    r_lo, r_hi = (n2 + 4) // 10, (19 * (n2 - 1) + 10) // 20
    cum, lo, hi = 0, None, None
    for j in gated:
        cum += n[j]
        if lo is None and cum > r_lo:
            lo = j
        if hi is None and cum > r_hi:
            hi = j
    return (float(centres[lo]), float(centres[hi]), float(gate), total, n2, lo, hi)


def records_of(hist):
    """counts [ns][751] -> RECORD [ns] by the rule"""
    centres = LL.tables()[2]
    out = np.zeros(len(hist), dtype=RECORD)
    for s, row in enumerate(hist):
        out[s] = range_rule(row, centres)
    return out


def lu(rec):
    return 0.1 * (int(rec["high_bin"]) - int(rec["low_bin"]))


class Oracle(LL.Oracle):
    """loudnesslib's oracle, with every short-term value it forms counted as a range block"""

    def __init__(self, cfgs):
        super().__init__(cfgs)
        self.hist_st = np.zeros((self.ns, NBINS), dtype=np.int64)

    def reset(self, s=-1):
        super().reset(s)
        self.hist_st[slice(None) if s < 0 else s] = 0

    def _close(self, s, ms0, ms1):
        super()._close(s, ms0, ms1)
        if len(self.z[s]) >= LL.RING:                                # a short-term value was formed: the record holds it
            st = self.rec[s]["short_term"]
            edges = LL.tables()[1]
            if st > edges[0]:
                self.hist_st[s, int(np.sum(st >= edges[1:]))] += 1

    def lra(self):
        return records_of(self.hist_st)


def signal(cfg, s, total, start=0):
    """int16 [2][total]: samples start .. start + total - 1 of stream s: a 997 Hz sine whose level steps every 23 frames through a staircase
    of its own between -6 and -38 dBFS (the second channel inverted); stream SILENT is digital silence, QUIET noise at -80 dBFS (measured,
    but nothing passes the absolute gate), CONSTANT a sine at -20 dBFS throughout.  The second row of a one-channel stream is filler."""
    if s == SILENT:
        return LL.signal(cfg, ("silence", 0.0), total, start=start)
    if s == QUIET:
        return LL.signal(cfg, ("noise", -80.0), total, seed=s, start=start)
    n = np.arange(start, start + total)
    step = n // (23 * N)
    db = -20.0 + 0.0 * step if s == CONSTANT else -6.0 - 4.0 * ((step * (s % 5 + 1) + s) % 9)
    v = np.round(32767.0 * 10.0 ** (db / 20.0) * np.sin(2.0 * math.pi * 997.0 * n / cfg["samplerate"]))
    v = np.clip(np.stack([v, -v]), -32768, 32767).astype(np.int16)
    if LL.nch_of(cfg) == 1:
        v[1] = 0x1111
    return v


def pcm_of(cfgs, nframes, f0=0):
    """the shared signals of frames f0 .. f0 + nframes - 1 as the ingest writes them: int16 [nframes][ns][2][1152]"""
    out = np.zeros((nframes, len(cfgs), 2, N), dtype=np.int16)
    for s, c in enumerate(cfgs):
        out[:, s] = signal(c, s, nframes * N, start=f0 * N).reshape(2, nframes, N).transpose(1, 0, 2)
    return out


def build_emu():
    """tests/emu/mp2_lra_emu.cpp -> a temporary directory, once per process (the flags of tests/emu/Makefile)"""
    return LL._build("libmp2lraemu.so", ["mp2_lra_emu.cpp"], ["-shared"])


def build_sanitized():
    """the same emulation behind tests/emu/lra_sanitize_main.cpp, a program of its own with AddressSanitizer + UBSan"""
    return LL._build("lra_sanitize", ["lra_sanitize_main.cpp", "mp2_lra_emu.cpp"], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def load_emu():
    L = C.CDLL(str(build_emu()))
    L.lra_loudness.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int]
    L.lra_range.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    assert L.lra_hist_rows() == HIST_ROWS and L.lra_lds_bytes() == 9216
    return L


def emu_range(hist):
    """counts [ns][751] -> RECORD [ns] through tl_lra_range on a [752][ns] array as the device keeps it"""
    h = np.zeros((HIST_ROWS, len(hist)), dtype=np.uint32)
    h[:NBINS] = np.asarray(hist, dtype=np.uint32).T
    out = np.zeros(len(hist), dtype=RECORD)
    rc = load_emu().lra_range(h.ctypes.data, len(hist), out.ctypes.data)
    assert rc == 0, rc
    return out


class LraEmu(LL.LoudnessEmu):
    """a stream set on the emulated kernels, the state held here as the batch's is on the device.  counting: the counting wave
    (tl_lra_kernel); else the plain one (tl_loudness_kernel), which is given no range counts at all"""

    def __init__(self, cfgs, counting=True):
        super().__init__(cfgs)
        self.X = load_emu()
        self.counting = counting
        self.hist_st = np.zeros((HIST_ROWS, self.ns), dtype=np.uint32)

    def reset(self, s=-1):
        super().reset(s)
        self.hist_st[:, slice(None) if s < 0 else slice(s, s + 1)] = 0

    def loudness(self, pcm):
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        assert a.shape[1:] == (self.ns, 2, N)
        out = np.zeros(self.ns, dtype=LL.RECORD)
        rc = self.X.lra_loudness(a.ctypes.data, a.shape[0], self.ns, self.nch.ctypes.data, self.rate.ctypes.data, self.lane.ctypes.data, self.ring.ctypes.data,
                                 self.rec.ctypes.data, self.hist.ctypes.data, self.hist_st.ctypes.data if self.counting else None, out.ctypes.data, int(self.counting))
        assert rc == 0, rc
        return out

    def lra(self):
        out = np.zeros(self.ns, dtype=RECORD)
        rc = self.X.lra_range(self.hist_st.ctypes.data, self.ns, out.ctypes.data)
        assert rc == 0, rc
        return out


same = LL.same
