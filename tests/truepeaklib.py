"""Support for the true-peak tests (test_truepeak_*.py): the definition of include/toolame_batch.h ("Maximum true peak", tlb_truepeak_*)
restated in numpy int64 -- the oracle, nothing else: a plain loop over the phases and taps of the definition on whole channels; it reads
the table through tlb_truepeak_taps and shares no code with the emulation -- the emulation of the kernel (tests/emu/mp2_truepeak_emu.cpp,
compiled into a temporary directory on first use, and the same text behind tests/emu/truepeak_sanitize_main.cpp with AddressSanitizer +
UBSan), and the constructed streams and signals the test files share."""
import ctypes as C
import math
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import loudnesslib as LL

ROOT = Path(__file__).resolve().parent.parent
N = 1152
T = 12
RECORD = np.dtype([("frames", "<u4"), ("overs", "<u4"), ("peak", "<u4", (2,)), ("peak_max", "<u4", (2,)), ("sample_max", "<u4", (2,))])
CEILING_DEFAULT = int(round(2.0 ** 30 * 10.0 ** (-1.0 / 20.0)))      # -1 dBTP
STREAMS = LL.STREAMS                                                 # 37 streams, all six rates, one and two channels
NFRAMES = LL.NFRAMES                                                 # 45
CUTS = LL.CUTS                                                       # one call, frame by frame, 7 + 38
nch_of = LL.nch_of
stream_configs = LL.stream_configs
same = LL.same


def dbtp(v):
    return 20.0 * math.log10(v / 2.0 ** 30) if v > 0 else -math.inf


_tab = {}


def taps():
    """the committed table through the library -> int64 [3][12]"""
    if "t" not in _tab:
        import odr_audioenc_amd as M
        if not M.LIB_PATH.exists():
            M.build()
        _tab["t"] = M.truepeak_taps().astype(np.int64)
    return _tab["t"]


def pcm_of(cfgs, nframes=NFRAMES, f0=0):
    """loudnesslib's shared signals (noise at four levels, a sine, silence, a full-scale square), int16 [nframes][ns][2][1152]"""
    return LL.pcm_of(cfgs, nframes, f0)


class Oracle:
    """the definition over a stream set: per channel the samples since the reset with T - 1 zeros ahead of them, v_p(n) as T shifted
    int64 products, the frame's peak as the maximum over its 1152 n"""

    def __init__(self, cfgs, ceiling=0):
        self.cfgs = [dict(c) for c in cfgs]
        self.ns = len(cfgs)
        self.ceiling = int(ceiling) if ceiling else CEILING_DEFAULT
        self.tail = np.zeros((self.ns, 2, T - 1), dtype=np.int64)    # x[-11 .. -1]
        self.rec = np.zeros(self.ns, dtype=RECORD)

    def reset(self, s=-1):
        for t in (range(self.ns) if s < 0 else (s,)):
            self.tail[t] = 0
            self.rec[t] = np.zeros((), dtype=RECORD)

    def reconfigure(self, s, cfg):
        self.cfgs[s] = dict(cfg)
        self.reset(s)

    def truepeak(self, pcm):
        """pcm int16 [nf][ns][2][1152] -> RECORD [ns] after these frames"""
        pcm = np.asarray(pcm)
        nf = pcm.shape[0]
        H = taps()
        for s in range(self.ns):
            r = self.rec[s]
            nch = nch_of(self.cfgs[s])
            peaks = np.zeros((nf, 2), dtype=np.int64)
            for c in range(nch):
                x = np.concatenate([self.tail[s, c], pcm[:, s, c].reshape(-1).astype(np.int64)])     # x[n] at index n + 11
                n = np.arange(nf * N) + (T - 1)
                v = [32768 * x[n]]
                for p in range(3):
                    acc = np.zeros(nf * N, dtype=np.int64)
                    for t in range(T):
                        acc += H[p, t] * x[n - t]
                    v.append(acc)
                peaks[:, c] = np.abs(np.stack(v)).max(axis=0).reshape(nf, N).max(axis=1)
                r["sample_max"][c] = max(int(r["sample_max"][c]), int(np.abs(x[T - 1:]).max()))
                self.tail[s, c] = x[-(T - 1):]
            assert peaks.max() < 2 ** 32
            for f in range(nf):
                r["frames"] += 1
                for c in range(nch):
                    r["peak"][c] = peaks[f, c]
                    r["peak_max"][c] = max(int(r["peak_max"][c]), int(peaks[f, c]))
                if peaks[f].max() > self.ceiling:
                    r["overs"] += 1
        return self.rec.copy()


GXX = LL.GXX
_emu = {}


def _build(name, sources, extra):
    if name not in _emu:
        d = Path(tempfile.mkdtemp(prefix="tpemu"))
        out = d / name
        subprocess.run(GXX + extra + ["-o", str(out)] + [str(ROOT / "tests" / "emu" / s) for s in sources] + ["-lm"], check=True)
        _emu[name] = out
    return _emu[name]


def build_emu():
    """tests/emu/mp2_truepeak_emu.cpp -> a temporary directory, once per process (the flags of tests/emu/Makefile)"""
    return _build("libmp2truepeakemu.so", ["mp2_truepeak_emu.cpp"], ["-shared"])


def build_sanitized():
    """the same emulation behind tests/emu/truepeak_sanitize_main.cpp, a program of its own with AddressSanitizer + UBSan"""
    return _build("truepeak_sanitize", ["truepeak_sanitize_main.cpp", "mp2_truepeak_emu.cpp"], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


class TruePeakEmu:
    """a stream set on the emulated kernel; the state lives here as the batch's lives on the device"""

    def __init__(self, cfgs, ceiling=0):
        L = self.L = C.CDLL(str(build_emu()))
        L.tp_truepeak.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.tp_carry() == 12
        self.cfgs = [dict(c) for c in cfgs]
        ns = self.ns = len(cfgs)
        self.ceiling = int(ceiling) if ceiling else CEILING_DEFAULT
        self.rec = np.zeros(ns, dtype=RECORD)
        self.hist = np.zeros((ns, 2, 6), dtype=np.uint32)
        self._cfg()

    def _cfg(self):
        self.nch = np.array([nch_of(c) for c in self.cfgs], dtype=np.int32)

    def reset(self, s=-1):
        sl = slice(None) if s < 0 else slice(s, s + 1)
        self.hist[sl] = 0
        self.rec[sl] = np.zeros((), dtype=RECORD)

    def reconfigure(self, s, cfg):
        self.cfgs[s] = dict(cfg)
        self._cfg()
        self.reset(s)

    def truepeak(self, pcm):
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        assert a.shape[1:] == (self.ns, 2, N)
        out = np.zeros(self.ns, dtype=RECORD)
        rc = self.L.tp_truepeak(a.ctypes.data, a.shape[0], self.ns, self.nch.ctypes.data, self.ceiling, self.rec.ctypes.data, self.hist.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out


# ---- the constructed cases: each the smallest input that catches one way of going wrong -----------------------------------------
def worst_case(p, sign):
    """T samples, oldest first, that drive phase p's sum to its largest magnitude: x[n - t] = -32768 where H[p][t] < 0 and 32767 elsewhere
    (sign -1: the other way round, 32767 where H[p][t] < 0 and -32768 elsewhere: the sum's negative extreme)"""
    h = taps()[p - 1]
    x = np.where(h < 0, -32768, 32767)
    if sign < 0:
        x = np.where(h < 0, 32767, -32768)
    return x[::-1].astype(np.int16)                                  # x[n - 11] .. x[n]


def constructed(nframes=3):
    """-> (cfgs, pcm int16 [nframes][ns][2][1152], names).  Two-channel streams unless said; all at 48 kHz (the arithmetic does not look at
    the rate)"""
    st, mo = dict(samplerate=48000, mode="s"), dict(samplerate=48000, mode="m")
    cfgs, rows, names = [], [], []

    def add(name, cfg, x):
        cfgs.append(cfg); rows.append(x); names.append(name)

    x = np.zeros((nframes, 2, N), dtype=np.int16); x[0, 0, N - 1] = 32767; x[0, 1, N - 1] = -32768
    add("impulse as the last sample of frame 0", st, x)
    x = np.zeros((nframes, 2, N), dtype=np.int16); x[1, 0, 0] = 32767; x[1, 1, 0] = -32768
    add("impulse as the first sample of frame 1", st, x)
    for p in (1, 2, 3):
        x = np.zeros((nframes, 2, N), dtype=np.int16)
        x[1, 0, 500:500 + T] = worst_case(p, 1); x[1, 1, 500:500 + T] = worst_case(p, -1)
        # once more across a frame boundary: seven samples in frame 1, five in frame 2
        x[1, 0, N - 7:] = worst_case(p, -1)[:7]; x[2, 0, :5] = worst_case(p, -1)[7:]
        add("worst case of phase %d" % p, st, x)
    x = np.zeros((nframes, 2, N), dtype=np.int16); x[:, 0] = 12345; x[:, 1] = 0x1234
    add("one channel, filler in the second row", mo, x)
    add("all zero", st, np.zeros((nframes, 2, N), dtype=np.int16))
    pcm = np.stack(rows, axis=1)
    return cfgs, pcm, names


def sine(freq_over_fs, phase, amp, n, fade=0):
    """round(32767 amp sin(2 pi f n + phase)), clipped to int16; fade: samples of raised-cosine fade in and out"""
    t = np.arange(n)
    s = amp * np.sin(2.0 * math.pi * freq_over_fs * t + phase)
    if fade:
        w = 0.5 - 0.5 * np.cos(math.pi * np.arange(fade) / fade)
        s[:fade] *= w
        s[-fade:] *= w[::-1]
    return np.clip(np.round(32767.0 * s), -32768, 32767).astype(np.int16)


def one_stream(x):
    """int16 [n] (n a multiple of 1152, else zero-padded) as a one-channel stream's PCM [nf][1][2][1152]"""
    nf = -(-len(x) // N)
    flat = np.zeros(nf * N, dtype=np.int16)
    flat[:len(x)] = x
    p = np.zeros((nf, 1, 2, N), dtype=np.int16)
    p[:, 0, 0] = flat.reshape(nf, N)
    return p
