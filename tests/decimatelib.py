"""Support for the decimator tests (test_decimate_*.py): the definition of include/toolame_batch.h ("Down sources", tlb_decimate_*) as a plain
loop over numpy int64 / Python ints -- the oracle, nothing else; it reads the table through tlb_decimate_taps and shares no code with the
emulation -- the emulation of the kernel (tests/emu/mp2_decimate_emu.cpp, compiled into a temporary directory on first use, and the same
text behind tests/emu/decimate_sanitize_main.cpp with AddressSanitizer + UBSan), and the stream set and inputs the test files share."""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from pcmgen import gen_pcm

ROOT = Path(__file__).resolve().parent.parent
N = 1152
T = 64
WIDE = 4608
# the smallest set with every ratio, both channel counts, a stream that is left alone and a second rate in the batch
STREAMS = [dict(samplerate=24000, mode="s", source=48000), dict(samplerate=24000, mode="m", source=48000),
           dict(samplerate=24000, mode="s", source=44100), dict(samplerate=24000, mode="m", source=32000),
           dict(samplerate=24000, mode="s", source=0), dict(samplerate=48000, mode="s", source=0)]
NFRAMES = 6                                                          # the need cycle of 80/147 is five frames: six pass its wrap
CUTS = ((6,), (1, 3, 2), (1, 1, 1, 1, 1, 1))
RATIOS = {48000: (1, 2), 32000: (3, 4), 44100: (80, 147)}
EMU_RATIO = {(80, 147): 1, (3, 4): 2, (1, 2): 3}                     # TL_DC_* of csrc/mp2_decimate.h
GXX = ["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
       "-Wno-unknown-pragmas", "-Wno-unused-but-set-variable", "-Wno-maybe-uninitialized"]


def nch_of(cfg):
    return 1 if cfg["mode"] == "m" else 2


def ratio_of(source, enc):
    return RATIOS.get(source) if enc == 24000 else None


def consumed(L, M, f):
    """S(f) = ceil(1152 f M / L): source frames consumed before frame f"""
    return -((-N * f * M) // L)


def need(source, enc, f):
    """need(f) of the header, in Python ints; 1152 without a down source"""
    if not source:
        return N
    L, M = ratio_of(source, enc)
    return consumed(L, M, f + 1) - consumed(L, M, f)


def total_need(cfg, nframes, f0=0):
    return sum(need(cfg["source"], cfg["samplerate"], f0 + f) for f in range(nframes))


_taps = {}


def taps(source, enc):
    """the committed table through tlb_decimate_taps -> int64 [L][64]"""
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    key = ratio_of(source, enc)
    if key not in _taps:
        H, L, Mm = M.decimate_taps(source, enc)
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
        q, p = (n * M + M - 1) // L, (n * M + M - 1) % L
        assert q < len(x), "the oracle was given too few source frames"
        seg = xp[q:q + T][::-1]                                      # x[q], x[q - 1], ..., x[q - 63]
        acc = (H[p][:, None] * seg).sum(axis=0)                      # exact in int64
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

    def decimate(self, wide, out=None):
        """wide int16 [nf][ns][4608] as tlb_decimate_device takes it -> int16 [nf][ns][2304]; what the call leaves unwritten keeps what
        `out` held (zeros without one)"""
        wide = np.asarray(wide)
        nf, ns = wide.shape[:2]
        out = np.zeros((nf, ns, 2 * N), dtype=np.int16) if out is None else out.copy()
        for s, c in enumerate(self.cfgs):
            nch = nch_of(c)
            for f in range(nf):
                if not c["source"]:
                    continue
                k = self.need(s)
                self.x[s] = np.concatenate([self.x[s], wide[f, s, :k * nch].astype(np.int64).reshape(k, nch)])
                y = oracle_stream(self.x[s], c["source"], c["samplerate"], N, n0=N * self.frames[s])
                out[f, s, :nch * N] = y.reshape(-1).astype(np.int16)
                self.frames[s] += 1
        return out


def signal(cfg, kind, total, seed=0):
    """a stream's source -> int16 [total][nch].  kind 'noise': pcmgen full-scale noise; 'square': full scale, period 64 source frames;
    ('const', c)"""
    nch = nch_of(cfg)
    if kind == "noise":
        v = gen_pcm(seed=700 + seed, kind=4, frame=0, nframes=(total + N - 1) // N)
        v = v.transpose(1, 0, 2).reshape(2, -1)[:nch, :total].T
    elif kind == "square":
        k = np.arange(total)
        v = np.repeat(np.where((k // 32) & 1, 32767, -32768)[:, None], nch, axis=1)
    else:
        v = np.full((total, nch), kind[1])
    return np.ascontiguousarray(v).astype(np.int16)


def signals(cfgs, kind, nframes=NFRAMES):
    return [signal(c, kind, total_need(c, nframes), seed=s) if c["source"] else None for s, c in enumerate(cfgs)]


def cut(sigs, cfgs, f0, nf, fill=0):
    """frames f0 .. f0 + nf - 1 of every down stream's signal as wide slots int16 [nf][ns][4608]; `fill` in every other value"""
    out = np.full((nf, len(cfgs), WIDE), fill, dtype=np.int16)
    for s, c in enumerate(cfgs):
        if not c["source"]:
            continue
        nch = nch_of(c)
        at = total_need(c, f0)
        for f in range(nf):
            k = need(c["source"], c["samplerate"], f0 + f)
            out[f, s, :k * nch] = sigs[s][at:at + k].reshape(-1)
            at += k
    return out


def background(nf, ns, seed=5):
    """what the output buffer holds before a call: the slots of streams without a down source (their own PCM) and the second half of a
    one-channel slot must come back as they were"""
    return np.random.default_rng(seed).integers(-32768, 32768, size=(nf, ns, 2 * N), dtype=np.int16)


def run_cuts(engine_decimate, sigs, cfgs, cuts, fill=0, bg=None):
    """the frames of `sigs` through engine_decimate(wide, out) cut by cut -> [sum(cuts)][ns][2304]"""
    outs, f0 = [], 0
    for n in cuts:
        o = None if bg is None else bg[f0:f0 + n].copy()
        outs.append(engine_decimate(cut(sigs, cfgs, f0, n, fill), o))
        f0 += n
    return np.concatenate(outs)


_emu = {}


def _build(name, sources, extra):
    if name not in _emu:
        d = Path(tempfile.mkdtemp(prefix="dcemu"))
        out = d / name
        subprocess.run(GXX + extra + ["-o", str(out)] + [str(ROOT / "tests" / "emu" / s) for s in sources] + ["-lm"], check=True)
        _emu[name] = out
    return _emu[name]


def build_emu():
    """tests/emu/mp2_decimate_emu.cpp -> a temporary directory, once per process (the flags of tests/emu/Makefile)"""
    return _build("libmp2decimateemu.so", ["mp2_decimate_emu.cpp"], ["-shared"])


def build_sanitized():
    """the same emulation behind tests/emu/decimate_sanitize_main.cpp, a program of its own with AddressSanitizer + UBSan"""
    return _build("decimate_sanitize", ["decimate_sanitize_main.cpp", "mp2_decimate_emu.cpp"], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


class DecimateEmu:
    """a stream set on the emulated kernel; the state and the flip live here as the batch's live on the device and in the host object"""

    def __init__(self, cfgs):
        L = self.L = C.CDLL(str(build_emu()))
        L.dc_decimate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert L.dc_state_words() == 64 and L.dc_table_rows() == 84
        self.cfgs = [dict(c) for c in cfgs]
        self.nch = np.array([nch_of(c) for c in cfgs], dtype=np.int32)
        self.ratio = np.array([EMU_RATIO[ratio_of(c["source"], c["samplerate"])] if c["source"] else 0 for c in cfgs], dtype=np.int32)
        self.state = np.zeros((2, len(cfgs), 64), dtype=np.uint32)
        self.flip = 0
        self.taps = np.concatenate([taps(r, 24000).reshape(-1) for r in (44100, 32000, 48000)]).astype(np.int16)

    def reset(self, s):
        self.state[:, s] = 0

    def decimate(self, wide, out=None):
        a = np.ascontiguousarray(wide, dtype=np.int16)
        nf, ns = a.shape[:2]
        assert a.shape == (nf, len(self.cfgs), WIDE)
        out = np.zeros((nf, ns, 2 * N), dtype=np.int16) if out is None else out
        rc = self.L.dc_decimate(a.ctypes.data, nf, ns, self.nch.ctypes.data, self.ratio.ctypes.data, self.state.ctypes.data, self.flip, self.taps.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        self.flip ^= 1
        return out


def adversarial(source, enc):
    """-> (x int16 [frames][1], n): a source that drives output n of a one-channel stream to the largest 32-bit quarter sum the table allows:
    x[q(n) - t] = -32768 sign(H[p][t]) over the row p with the largest sum |H| of a 16-tap quarter (every tap of the row, so that all four
    quarters are at their extreme and the whole-row sum is far outside 32 bits)"""
    L, M = ratio_of(source, enc)
    H = taps(source, enc)
    p = int(np.abs(H).reshape(L, 4, 16).sum(axis=2).max(axis=1).argmax())
    n = next(n for n in range(200, 200 + 2 * L + 2) if (n * M + M - 1) % L == p)
    q = (n * M + M - 1) // L
    x = np.zeros((q + 1, 1), dtype=np.int64)
    for t in range(T):
        x[q - t, 0] = -32768 if H[p][t] > 0 else 32767 if H[p][t] < 0 else 0
    return x.astype(np.int16), n, p


def stream_configs(cfgs, kbps=None):
    """the set as odr_audioenc_amd.StreamConfig records"""
    import odr_audioenc_amd as M
    return [M.StreamConfig(samplerate=c["samplerate"], mode=c["mode"], bitrate=c.get("kbps", kbps or (128 if c["samplerate"] == 48000 else 64)), psy_model=c.get("psy", 1)) for c in cfgs]
