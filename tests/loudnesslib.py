"""Support for the loudness tests (test_loudness_*.py): the definition of include/toolame_batch.h ("Programme loudness", tlb_loudness_*)
restated in numpy -- the oracle, nothing else: vectorised over the (stream, channel) lanes so that its Python loop runs over the samples
once; it reads the table through tlb_loudness_taps / tlb_loudness_scale and shares no code with the emulation -- the emulation of the
kernels (tests/emu/mp2_loudness_emu.cpp, compiled into a temporary directory on first use, and the same text behind
tests/emu/loudness_sanitize_main.cpp with AddressSanitizer + UBSan), and the stream set and signals the test files share."""
import ctypes as C
import math
import subprocess
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
N = 1152
RATES = (48000, 44100, 32000, 24000, 22050, 16000)
RING = 30
NBINS = 751
HIST_ROWS = 752
RECORD = np.dtype([("frames", "<u4"), ("bins", "<u4"), ("blocks", "<u4"), ("gated", "<u4"),
                   ("momentary", "<f8"), ("short_term", "<f8"), ("momentary_max", "<f8"), ("short_term_max", "<f8")])
PROGRAMME = np.dtype([("integrated", "<f8"), ("gate", "<f8"), ("gated", "<u4"), ("reserved", "<u4")])
# 37 streams = 74 lanes: a full wave and a second one with five streams; every rate with one and with two channels
STREAMS = [dict(samplerate=RATES[s % 6], mode="m" if (s // 6 + s) % 2 else "s") for s in range(37)]
NFRAMES = 45                                                         # 51 840 samples: 32 bins at 16 kHz (short-term exists), 10 at 48 kHz
CUTS = ((45,), (1,) * 45, (7, 38))
KINDS = (("noise", 0.0), ("noise", -20.0), ("sine", 0.0), ("silence", 0.0), ("square", 0.0), ("noise", -45.0), ("noise", -80.0))
GXX = ["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
       "-Wno-unknown-pragmas", "-Wno-unused-but-set-variable", "-Wno-maybe-uninitialized"]


def nch_of(cfg):
    return 1 if cfg["mode"] == "m" else 2


def lufs(e):
    return -0.691 + 10.0 * math.log10(e) if e > 0 else -math.inf


_tab = {}


def tables():
    """the committed table through the library -> (taps {rate: float64 [10]}, edges [751], centres [751])"""
    if not _tab:
        import odr_audioenc_amd as M
        if not M.LIB_PATH.exists():
            M.build()
        edges, centres = M.loudness_scale()
        _tab["t"] = ({r: M.loudness_taps(r) for r in RATES}, edges, centres)
    return _tab["t"]


class Oracle:
    """the definition over a stream set: numpy float64 elementwise operations in the order the header writes them (every one a single
    correctly rounded IEEE operation), one Python step per sample for all lanes together"""

    def __init__(self, cfgs):
        self.cfgs = [dict(c) for c in cfgs]
        ns = self.ns = len(cfgs)
        self.q = np.zeros((8, 2 * ns))
        self.acc = np.zeros(2 * ns)
        self.pos = np.zeros(2 * ns, dtype=np.int64)
        self.z = [[] for _ in range(ns)]                             # every closed bin since the reset
        self.hist = np.zeros((ns, NBINS), dtype=np.int64)
        self.rec = np.zeros(ns, dtype=RECORD)
        self._coefs()

    def _coefs(self):
        taps = tables()[0]
        self.k = np.stack([np.repeat(np.array([taps[c["samplerate"]][i] for c in self.cfgs]), 2) for i in range(10)])
        self.binlen = np.repeat(np.array([c["samplerate"] // 10 for c in self.cfgs], dtype=np.int64), 2)

    def reset(self, s=-1):
        for t in (range(self.ns) if s < 0 else (s,)):
            self.q[:, 2 * t:2 * t + 2] = 0.0
            self.acc[2 * t:2 * t + 2] = 0.0
            self.pos[2 * t:2 * t + 2] = 0
            self.z[t] = []
            self.hist[t] = 0
            self.rec[t] = np.zeros((), dtype=RECORD)

    def reconfigure(self, s, cfg):
        self.cfgs[s] = dict(cfg)
        self._coefs()
        self.reset(s)

    def _close(self, s, ms0, ms1):
        edges = tables()[1]
        r = self.rec[s]
        z = ms0 + ms1 if nch_of(self.cfgs[s]) == 2 else ms0
        zs = self.z[s]
        zs.append(z)
        r["bins"] += 1
        if len(zs) >= 4:
            m = (((zs[-4] + zs[-3]) + zs[-2]) + zs[-1]) * 0.25
            r["blocks"] += 1
            r["momentary"] = m
            if m > r["momentary_max"]:
                r["momentary_max"] = m
            if m > edges[0]:
                self.hist[s, int(np.sum(m >= edges[1:]))] += 1
                r["gated"] += 1
        if len(zs) >= RING:
            t = zs[-RING]
            for v in zs[-RING + 1:]:
                t = t + v
            st = t / 30.0
            r["short_term"] = st
            if st > r["short_term_max"]:
                r["short_term_max"] = st

    def loudness(self, pcm):
        """pcm int16 [nf][ns][2][1152] -> RECORD [ns] after these frames"""
        pcm = np.asarray(pcm)
        nf = pcm.shape[0]
        x_all = pcm.transpose(1, 2, 0, 3).reshape(2 * self.ns, nf * N).astype(np.float64) * (1.0 / 32768.0)
        q, k = self.q, self.k
        for n in range(nf * N):
            x = x_all[:, n]
            t = ((k[0] * x) + (k[1] * q[0])) + (k[2] * q[1])
            y = (t - (k[4] * q[3])) - (k[3] * q[2])
            q[1] = q[0]; q[0] = x; q[3] = q[2]; q[2] = y
            t = ((k[5] * y) + (k[6] * q[4])) + (k[7] * q[5])
            y2 = (t - (k[9] * q[7])) - (k[8] * q[6])
            q[5] = q[4]; q[4] = y; q[7] = q[6]; q[6] = y2
            self.acc = self.acc + (y2 * y2)
            self.pos += 1
            full = self.pos == self.binlen
            if full.any():
                ms = self.acc / self.binlen.astype(np.float64)
                for s in np.nonzero(full[0::2])[0]:
                    self._close(int(s), float(ms[2 * s]), float(ms[2 * s + 1]))
                self.acc[full] = 0.0
                self.pos[full] = 0
        self.rec["frames"] += nf
        return self.rec.copy()

    def programme(self):
        centres = tables()[2]
        out = np.zeros(self.ns, dtype=PROGRAMME)
        for s in range(self.ns):
            n_tot, S = 0, 0.0
            for j in range(NBINS):
                n_tot += int(self.hist[s, j]); S = S + float(self.hist[s, j]) * centres[j]
            if not n_tot:
                continue
            gate = 0.1 * (S / float(n_tot))
            n2, S2 = 0, 0.0
            for j in range(NBINS):
                if centres[j] >= gate:
                    n2 += int(self.hist[s, j]); S2 = S2 + float(self.hist[s, j]) * centres[j]
            out[s] = (S2 / float(n2), gate, n2, 0)
        return out


def signal(cfg, kind, total, seed=0, start=0):
    """int16 [2][total]: samples start .. start + total - 1 of a stream's signal; the second row of a one-channel stream is filler the
    meter must not read into anything (0x1111).  kind: ('noise', dBFS peak), ('sine', dBFS) 997 Hz, ('silence', .), ('square', .) full
    scale +32767 / -32768 with a period of 48 samples"""
    name, db = kind
    n = np.arange(start, start + total)
    a = 10.0 ** (db / 20.0)
    if name == "noise":
        rng = np.random.default_rng(900 + seed)
        v = np.floor(rng.uniform(-32768.0 * a, 32767.0 * a + 1.0, size=(2, start + total)))[:, start:]
    elif name == "sine":
        v = np.round(32767.0 * a * np.sin(2.0 * math.pi * 997.0 * n / cfg["samplerate"]))
        v = np.stack([v, -v])
    elif name == "square":
        v = np.where((n // 24) & 1, 32767, -32768)
        v = np.stack([v, v])
    else:
        v = np.zeros((2, total))
    v = np.clip(v, -32768, 32767).astype(np.int16)
    if nch_of(cfg) == 1:
        v[1] = 0x1111
    return v


def pcm_of(cfgs, nframes=NFRAMES, f0=0):
    """the shared signals of frames f0 .. f0 + nframes - 1 as the ingest writes them: int16 [nframes][ns][2][1152]"""
    out = np.zeros((nframes, len(cfgs), 2, N), dtype=np.int16)
    for s, c in enumerate(cfgs):
        v = signal(c, KINDS[s % len(KINDS)], nframes * N, seed=s, start=f0 * N)
        out[:, s] = v.reshape(2, nframes, N).transpose(1, 0, 2)
    return out


def run_cuts(engine, pcm, cuts):
    """engine.loudness over pcm cut by cut -> the records after every cut"""
    recs, f0 = [], 0
    for n in cuts:
        recs.append(engine.loudness(pcm[f0:f0 + n]))
        f0 += n
    return recs


_emu = {}


def _build(name, sources, extra):
    if name not in _emu:
        d = Path(tempfile.mkdtemp(prefix="ldemu"))
        out = d / name
        subprocess.run(GXX + extra + ["-o", str(out)] + [str(ROOT / "tests" / "emu" / s) for s in sources] + ["-lm"], check=True)
        _emu[name] = out
    return _emu[name]


def build_emu():
    """tests/emu/mp2_loudness_emu.cpp -> a temporary directory, once per process (the flags of tests/emu/Makefile)"""
    return _build("libmp2loudnessemu.so", ["mp2_loudness_emu.cpp"], ["-shared"])


def build_sanitized():
    """the same emulation behind tests/emu/loudness_sanitize_main.cpp, a program of its own with AddressSanitizer + UBSan"""
    return _build("loudness_sanitize", ["loudness_sanitize_main.cpp", "mp2_loudness_emu.cpp"], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


class LoudnessEmu:
    """a stream set on the emulated kernels; the state lives here as the batch's lives on the device"""

    def __init__(self, cfgs):
        L = self.L = C.CDLL(str(build_emu()))
        L.ld_loudness.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        L.ld_programme.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        assert L.ld_lane_words() == 10 and L.ld_hist_rows() == HIST_ROWS
        self.cfgs = [dict(c) for c in cfgs]
        ns = self.ns = len(cfgs)
        self.lane = np.zeros((10, 2 * ns))
        self.ring = np.zeros((RING, ns))
        self.rec = np.zeros(ns, dtype=RECORD)
        self.hist = np.zeros((HIST_ROWS, ns), dtype=np.uint32)
        self._cfg()

    def _cfg(self):
        self.nch = np.array([nch_of(c) for c in self.cfgs], dtype=np.int32)
        self.rate = np.array([c["samplerate"] for c in self.cfgs], dtype=np.int32)

    def reset(self, s=-1):
        sl = slice(None) if s < 0 else slice(s, s + 1)
        self.lane[:, (slice(None) if s < 0 else slice(2 * s, 2 * s + 2))] = 0.0
        self.ring[:, sl] = 0.0
        self.hist[:, sl] = 0
        self.rec[sl] = np.zeros((), dtype=RECORD)

    def reconfigure(self, s, cfg):
        self.cfgs[s] = dict(cfg)
        self._cfg()
        self.reset(s)

    def loudness(self, pcm):
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        assert a.shape[1:] == (self.ns, 2, N)
        out = np.zeros(self.ns, dtype=RECORD)
        rc = self.L.ld_loudness(a.ctypes.data, a.shape[0], self.ns, self.nch.ctypes.data, self.rate.ctypes.data, self.lane.ctypes.data,
                                self.ring.ctypes.data, self.rec.ctypes.data, self.hist.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out

    def programme(self):
        out = np.zeros(self.ns, dtype=PROGRAMME)
        rc = self.L.ld_programme(self.hist.ctypes.data, self.ns, out.ctypes.data)
        assert rc == 0, rc
        return out


def same(a, b):
    """two record arrays bit for bit (the doubles as their bytes: -0.0 and NaN payloads count)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def stream_configs(cfgs):
    """the set as odr_audioenc_amd.StreamConfig records"""
    import odr_audioenc_amd as M
    return [M.StreamConfig(samplerate=c["samplerate"], mode=c["mode"], bitrate=c.get("kbps", 128 if c["samplerate"] >= 32000 else 64), psy_model=c.get("psy", 1)) for c in cfgs]
