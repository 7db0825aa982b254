"""Support for the resampler tests (test_resample_*.py): the two formulas of include/toolame_batch.h (tlb_resample_*) as a plain loop over
numpy int64 -- the oracle, nothing else; it reads the table through tlb_resample_taps and shares no code with the emulation -- the
emulation of the kernel (tests/emu/mp2_resample_emu.cpp, compiled into a temporary directory on first use), and the stream set and
inputs the test files share."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from pcmgen import gen_pcm

ROOT = Path(__file__).resolve().parent.parent
N = 1152
T = 32
# the issue's five streams: both ratios at both encoder rates, one and two channels, and one stream without a source
STREAMS = [dict(samplerate=48000, mode="s", source=44100), dict(samplerate=48000, mode="m", source=32000),
           dict(samplerate=24000, mode="m", source=22050), dict(samplerate=24000, mode="s", source=16000),
           dict(samplerate=48000, mode="s", source=0)]
NFRAMES = 6                                                          # the need cycle is five frames: six pass its wrap
CUTS = ((6,), (1, 3, 2), (1, 1, 1, 1, 1, 1))


def nch_of(cfg):
    return 1 if cfg["mode"] == "m" else 2


def ratio_of(source, enc):
    if (source, enc) in ((44100, 48000), (22050, 24000)):
        return 160, 147
    if (source, enc) in ((32000, 48000), (16000, 24000)):
        return 3, 2
    return None


def q_of(n, L, M):
    return (n * M) // L


def need(source, enc, f):
    """need(f) of the header, in Python ints; 1152 without a source"""
    if not source:
        return N
    L, M = ratio_of(source, enc)
    return q_of(N * (f + 1) - 1, L, M) + 1 - (q_of(N * f - 1, L, M) + 1 if f > 0 else 0)


def total_need(cfg, nframes, f0=0):
    return sum(need(cfg["source"], cfg["samplerate"], f0 + f) for f in range(nframes))


_taps = {}


def taps(source, enc):
    """the committed table through tlb_resample_taps -> int64 [L][32]"""
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    key = ratio_of(source, enc)
    if key not in _taps:
        H, L, Mm = M.resample_taps(source, enc)
        assert (L, Mm) == key and H.shape == (L, T)
        _taps[key] = H.astype(np.int64)
    return _taps[key]


def oracle_stream(x, source, enc, nout, n0=0, unclamped=False):
    """x int [frames since the reset][nch] -> y int64 [nout][nch], outputs n0 .. n0 + nout - 1 of the stream: the definition"""
    L, M = ratio_of(source, enc)
    H = taps(source, enc)
    x = np.asarray(x, dtype=np.int64)
    xp = np.concatenate([np.zeros((T - 1, x.shape[1]), dtype=np.int64), x])      # x[j] = 0 for j < 0
    out = np.zeros((nout, x.shape[1]), dtype=np.int64)
    for i in range(nout):
        n = n0 + i
        q, p = (n * M) // L, (n * M) % L
        assert q < len(x), "the oracle was given too few source frames"
        seg = xp[q:q + T][::-1]                                      # x[q], x[q - 1], ..., x[q - 31]
        acc = (H[p][:, None] * seg).sum(axis=0)                      # exact: |acc| < 2^32 in int64
        out[i] = acc if unclamped else np.clip((acc + 16384) >> 15, -32768, 32767)
    return out


class Oracle:
    """every stream of a set from its reset on: keeps each stream's whole source and its output count"""

    def __init__(self, cfgs):
        self.cfgs = [dict(c) for c in cfgs]
        self.x = [np.zeros((0, nch_of(c)), dtype=np.int64) for c in cfgs]
        self.frames = [0] * len(cfgs)

    def reset(self, s):
        self.x[s] = np.zeros((0, nch_of(self.cfgs[s])), dtype=np.int64)
        self.frames[s] = 0

    def need(self, s, ahead=0):
        c = self.cfgs[s]
        return need(c["source"], c["samplerate"], self.frames[s] + ahead)

    def resample(self, slots):
        """slots int16 [nf][ns][2304] as tlb_resample_device takes them -> the same shape; what the call leaves unwritten is 0"""
        slots = np.asarray(slots)
        nf, ns = slots.shape[:2]
        out = np.zeros((nf, ns, 2 * N), dtype=np.int16)
        for s, c in enumerate(self.cfgs):
            nch = nch_of(c)
            for f in range(nf):
                if not c["source"]:
                    out[f, s, :nch * N] = slots[f, s, :nch * N]
                    continue
                k = self.need(s)
                self.x[s] = np.concatenate([self.x[s], slots[f, s, :k * nch].astype(np.int64).reshape(k, nch)])
                y = oracle_stream(self.x[s], c["source"], c["samplerate"], N, n0=N * self.frames[s])
                out[f, s, :nch * N] = y.reshape(-1).astype(np.int16)
                self.frames[s] += 1
        return out


def defined(cfgs):
    """bool [ns][2304]: the values of an output slot the call writes (a one-channel stream: the first 1152)"""
    m = np.zeros((len(cfgs), 2 * N), dtype=bool)
    for s, c in enumerate(cfgs):
        m[s, :nch_of(c) * N] = True
    return m


def same(got, want, cfgs, what=""):
    m = defined(cfgs)
    for s in range(len(cfgs)):
        g, w = np.asarray(got)[:, s][:, m[s]], np.asarray(want)[:, s][:, m[s]]
        assert np.array_equal(g, w), (what, "stream", s, "first difference at", np.argwhere(g != w)[:4].tolist())


def signal(cfg, kind, total, seed=0):
    """a stream's source (or, without a source, its encoder-rate PCM) -> int16 [total][nch]
    kind 'noise': pcmgen full-scale noise; 'square': full scale, period 64 source frames; ('const', c); ('sine', hz, amplitude)"""
    nch = nch_of(cfg)
    if kind == "noise":
        v = gen_pcm(seed=900 + seed, kind=4, frame=0, nframes=(total + N - 1) // N)
        v = v.transpose(1, 0, 2).reshape(2, -1)[:nch, :total].T
    elif kind == "square":
        k = np.arange(total)
        v = np.repeat(np.where((k // 32) & 1, 32767, -32768)[:, None], nch, axis=1)
    elif kind[0] == "const":
        v = np.full((total, nch), kind[1])
    else:
        rate = cfg["source"] or cfg["samplerate"]
        k = np.arange(total, dtype=np.float64)
        v = np.repeat(np.round(kind[2] * np.sin(2 * np.pi * kind[1] * k / rate))[:, None], nch, axis=1)
    return np.ascontiguousarray(v).astype(np.int16)


def cut(sigs, cfgs, f0, nf, fill=0):
    """frames f0 .. f0 + nf - 1 of every stream's signal as slots int16 [nf][ns][2304]; `fill` in every value behind the need frames"""
    out = np.full((nf, len(cfgs), 2 * N), fill, dtype=np.int16)
    for s, c in enumerate(cfgs):
        nch = nch_of(c)
        at = total_need(c, f0)
        for f in range(nf):
            k = need(c["source"], c["samplerate"], f0 + f)
            out[f, s, :k * nch] = sigs[s][at:at + k].reshape(-1)
            at += k
    return out


def signals(cfgs, kind, nframes=NFRAMES):
    return [signal(c, kind, total_need(c, nframes), seed=s) for s, c in enumerate(cfgs)]


_emu_so = None


def build_emu():
    """tests/emu/mp2_resample_emu.cpp -> a temporary directory, once per process (the flags of tests/emu/Makefile)"""
    global _emu_so
    if _emu_so is None:
        import tempfile
        d = Path(tempfile.mkdtemp(prefix="rsemu"))
        so = d / "libmp2resampleemu.so"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function",
                        "-Wno-unused-variable", "-Wno-unknown-pragmas", "-Wno-unused-but-set-variable", "-Wno-maybe-uninitialized", "-shared", "-o", str(so),
                        str(ROOT / "tests" / "emu" / "mp2_resample_emu.cpp"), "-lm"], check=True)
        _emu_so = so
    return _emu_so


class ResampleEmu:
    """a stream set on the emulated kernel; the state and the flip live here as the batch's live on the device and in the host object"""

    def __init__(self, cfgs):
        L = self.L = C.CDLL(str(build_emu()))
        L.rs_resample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert L.rs_state_words() == 32
        self.cfgs = [dict(c) for c in cfgs]
        self.nch = np.array([nch_of(c) for c in cfgs], dtype=np.int32)
        self.ratio = np.array([{None: 0, (160, 147): 1, (3, 2): 2}[ratio_of(c["source"], c["samplerate"]) if c["source"] else None] for c in cfgs], dtype=np.int32)
        self.state = np.zeros((2, len(cfgs), 32), dtype=np.uint32)
        self.flip = 0
        self.taps = np.concatenate([taps(44100, 48000).reshape(-1), taps(32000, 48000).reshape(-1)]).astype(np.int16)

    def reset(self, s):
        self.state[:, s] = 0

    def resample(self, slots, out=None):
        a = np.ascontiguousarray(slots, dtype=np.int16)
        nf, ns = a.shape[:2]
        assert a.shape == (nf, len(self.cfgs), 2 * N)
        out = np.zeros_like(a) if out is None else out
        rc = self.L.rs_resample(a.ctypes.data, nf, ns, self.nch.ctypes.data, self.ratio.ctypes.data, self.state.ctypes.data, self.flip, self.taps.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        self.flip ^= 1
        return out


def run_cuts(engine_resample, sigs, cfgs, cuts, fill=0):
    """the frames of `sigs` through engine_resample(slots) cut by cut -> [sum(cuts)][ns][2304]"""
    outs, f0 = [], 0
    for n in cuts:
        outs.append(engine_resample(cut(sigs, cfgs, f0, n, fill)))
        f0 += n
    return np.concatenate(outs)


def stream_configs(cfgs, kbps=None):
    """the set as odr_audioenc_amd.StreamConfig records"""
    import odr_audioenc_amd as M
    return [M.StreamConfig(samplerate=c["samplerate"], mode=c["mode"], bitrate=c.get("kbps", kbps or (128 if c["samplerate"] == 48000 else 64)), psy_model=c.get("psy", 1)) for c in cfgs]
