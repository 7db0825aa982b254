"""Support for the limiter tests (test_limiter_*.py): the definition of include/toolame_batch.h ("True-peak limiter", tlb_limiter_*)
restated in numpy int64 -- the oracle, nothing else: the six steps of the definition on whole channels, one after the other; it reads
the table through tlb_truepeak_taps and shares no code with the emulation -- the emulation of the kernel (tests/emu/mp2_limiter_emu.cpp,
compiled into a temporary directory on first use, and the same text behind tests/emu/limiter_sanitize_main.cpp with AddressSanitizer +
UBSan), and the constructed streams and signals the test files share."""
import ctypes as C
import math

import numpy as np

import loudnesslib as LL
import truepeaklib as TP

N = 1152
T = 12
U = 1 << 30
WMIN, WBOX, DELAY = 64, 32, 63
RECORD = np.dtype([("frames", "<u4"), ("limited", "<u4"), ("samples", "<u4"), ("red_last", "<u4"), ("red_max", "<u4"),
                   ("peak_in", "<u4"), ("peak_in_max", "<u4"), ("reserved", "<u4")])
CEILING_DEFAULT = TP.CEILING_DEFAULT
RELEASE_DEFAULT_MS = 100
STREAMS = LL.STREAMS
NFRAMES = LL.NFRAMES
CUTS = LL.CUTS
nch_of = LL.nch_of
same = LL.same
taps = TP.taps
STATE_WORDS = 172                                                    # uint32 per stream beside the record (csrc/mp2_limiter.h)


def step(release_ms, samplerate):
    """tlb_limiter_step: the gain's recovery per sample, max(1, (2^30 * 1000) / (release_ms * samplerate)); 0 ms is the default"""
    ms = release_ms if release_ms else RELEASE_DEFAULT_MS
    return max(1, (U * 1000) // (ms * samplerate))


def release_serial(m, S, e_prev):
    """step 4 as the recurrence itself, one sample after the other (the closed form the oracle uses is checked against it)"""
    e = np.empty(len(m), dtype=np.int64)
    for n in range(len(m)):
        e_prev = min(int(m[n]), min(U, e_prev + S))
        e[n] = e_prev
    return e


class Oracle:
    """the definition over a stream set.  Per stream it keeps what the definition reaches back to: the last 74 samples of either channel
    (63 of delay, 11 of taps), r[-63 .. -1], e[-31 .. -1]; all unity / zero after a reset"""

    def __init__(self, cfgs, ceiling=0, release_ms=0, steps=None):
        self.cfgs = [dict(c) for c in cfgs]
        self.ns = len(cfgs)
        self.ceiling = int(ceiling) if ceiling else CEILING_DEFAULT
        self.release_ms = int(release_ms)
        self.steps = None if steps is None else [int(v) for v in steps]      # the tests of the theorem give S directly
        self.rec = np.zeros(self.ns, dtype=RECORD)
        self.xt = np.zeros((self.ns, 2, DELAY + T - 1), dtype=np.int64)
        self.rt = np.full((self.ns, WMIN - 1), U, dtype=np.int64)
        self.et = np.full((self.ns, WBOX - 1), U, dtype=np.int64)
        self.gains = [None] * self.ns                                # G of the last call, per stream (for the tests' own assertions)

    def S(self, s):
        return self.steps[s] if self.steps is not None else step(self.release_ms, self.cfgs[s]["samplerate"])

    def reset(self, s=-1):
        for t in (range(self.ns) if s < 0 else (s,)):
            self.xt[t] = 0
            self.rt[t] = U
            self.et[t] = U
            self.rec[t] = np.zeros((), dtype=RECORD)

    def reconfigure(self, s, cfg):
        self.cfgs[s] = dict(cfg)
        self.reset(s)

    def limit(self, pcm):
        """pcm int16 [nf][ns][2][1152] -> (limited pcm, RECORD [ns] after these frames)"""
        pcm = np.asarray(pcm)
        nf = pcm.shape[0]
        out = pcm.copy()
        H = taps()
        K = DELAY + T - 1
        for s in range(self.ns):
            nch = nch_of(self.cfgs[s])
            S = self.S(s)
            tot = nf * N
            xs = [np.concatenate([self.xt[s, c], pcm[:, s, c].reshape(-1).astype(np.int64)]) for c in range(nch)]     # x[n] at index n + K
            n = np.arange(tot) + K
            # 1. detector
            P = np.zeros(tot, dtype=np.int64)
            for x in xs:
                P = np.maximum(P, 32768 * np.abs(x[n]))
                for p in range(3):
                    acc = np.zeros(tot, dtype=np.int64)
                    for t in range(T):
                        acc += H[p, t] * x[n - t]
                    P = np.maximum(P, np.abs(acc))
            assert P.max() < 2 ** 32
            # 2. required gain (Python integers: the product needs 64 bits and numpy's would do, but so it is beyond doubt)
            r = np.full(tot, U, dtype=np.int64)
            for i in np.nonzero(P > self.ceiling)[0]:
                r[i] = (self.ceiling << 30) // int(P[i])
            # 3. hold
            rr = np.concatenate([self.rt[s], r])
            m = np.lib.stride_tricks.sliding_window_view(rr, WMIN).min(axis=1)
            # 4. release, in the closed form: e[n] = min(U, min_{k <= n}(m[k] + (n - k) S), e[-1] + (n + 1) S)
            k = np.arange(tot, dtype=np.int64)
            e = np.minimum(U, np.minimum(np.minimum.accumulate(m - k * S) + k * S, int(self.et[s, -1]) + (k + 1) * S))
            # 5. smooth
            ee = np.concatenate([self.et[s], e])
            cs = np.concatenate([[0], np.cumsum(ee)])
            G = (cs[WBOX:] - cs[:-WBOX]) >> 19
            assert len(G) == tot and G.min() >= 0 and G.max() <= 65536
            # 6. apply
            for c, x in enumerate(xs):
                d = x[n - DELAY]
                y = np.sign(d) * ((np.abs(d) * G) >> 16)
                out[:, s, c] = y.reshape(nf, N).astype(np.int16)
                self.xt[s, c] = x[-K:]
            self.rt[s] = rr[-(WMIN - 1):]
            self.et[s] = ee[-(WBOX - 1):]
            self.gains[s] = G
            rec = self.rec[s]
            Gf, Pf = G.reshape(nf, N), P.reshape(nf, N)
            for f in range(nf):
                cnt = int((Gf[f] < 65536).sum())
                rec["frames"] += 1
                rec["limited"] += 1 if cnt else 0
                rec["samples"] = min(0xffffffff, int(rec["samples"]) + cnt)
                rec["red_last"] = 65536 - int(Gf[f].min())
                rec["red_max"] = max(int(rec["red_max"]), int(rec["red_last"]))
                rec["peak_in"] = int(Pf[f].max())
                rec["peak_in_max"] = max(int(rec["peak_in_max"]), int(rec["peak_in"]))
        return out, self.rec.copy()


_build = TP._build


def build_emu():
    """tests/emu/mp2_limiter_emu.cpp -> a temporary directory, once per process (the flags of tests/emu/Makefile)"""
    return _build("libmp2limiteremu.so", ["mp2_limiter_emu.cpp"], ["-shared"])


def build_sanitized():
    """the same emulation behind tests/emu/limiter_sanitize_main.cpp, a program of its own with AddressSanitizer + UBSan"""
    return _build("limiter_sanitize", ["limiter_sanitize_main.cpp", "mp2_limiter_emu.cpp"], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


class LimiterEmu:
    """a stream set on the emulated kernel; the state lives here as the batch's lives on the device"""

    def __init__(self, cfgs, ceiling=0, release_ms=0, steps=None):
        L = self.L = C.CDLL(str(build_emu()))
        L.lm_limit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lm_paths.argtypes = [C.c_void_p]
        assert L.lm_state_words() == STATE_WORDS
        self.cfgs = [dict(c) for c in cfgs]
        ns = self.ns = len(cfgs)
        self.ceiling = int(ceiling) if ceiling else CEILING_DEFAULT
        self.release_ms = int(release_ms)
        self.steps = None if steps is None else [int(v) for v in steps]
        self.rec = np.zeros(ns, dtype=RECORD)
        self.state = np.zeros((ns, STATE_WORDS), dtype=np.uint32)
        self.paths = np.zeros(2, dtype=np.int64)
        self._cfg()

    def _cfg(self):
        self.nch = np.array([nch_of(c) for c in self.cfgs], dtype=np.int32)
        self.S = np.array([self.steps[s] if self.steps is not None else step(self.release_ms, c["samplerate"]) for s, c in enumerate(self.cfgs)], dtype=np.uint32)

    def reset(self, s=-1):
        sl = slice(None) if s < 0 else slice(s, s + 1)
        self.state[sl] = 0
        self.rec[sl] = np.zeros((), dtype=RECORD)

    def reconfigure(self, s, cfg):
        self.cfgs[s] = dict(cfg)
        self._cfg()
        self.reset(s)

    def limit(self, pcm):
        a = np.array(pcm, dtype=np.int16, order="C")                 # a copy: the kernel works in place
        assert a.shape[1:] == (self.ns, 2, N)
        out = np.zeros(self.ns, dtype=RECORD)
        rc = self.L.lm_limit(a.ctypes.data, a.shape[0], self.ns, self.nch.ctypes.data, self.S.ctypes.data, self.ceiling, self.rec.ctypes.data, self.state.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return a, out

    def path_counts(self):
        """(frames on the idle path, frames on the active path) since the library was loaded"""
        self.L.lm_paths(self.paths.ctypes.data)
        return int(self.paths[0]), int(self.paths[1])


# ---- signals ---------------------------------------------------------------------------------------------------------------------
def pcm_of(cfgs, nframes=NFRAMES, f0=0):
    return LL.pcm_of(cfgs, nframes, f0)


def frames_of(x):
    """int16 [n] zero-padded to whole frames -> [nf][1152]"""
    nf = -(-len(x) // N)
    flat = np.zeros(nf * N, dtype=np.int16)
    flat[:len(x)] = x
    return flat.reshape(nf, N)


def constructed(nframes=4):
    """-> (cfgs, pcm int16 [nframes][6][2][1152], names): the six streams of the device test, each with one constructed case (or two).
    The background is a quiet sine (amplitude 3000: far below any ceiling used), so a gain below unity shows in every output sample"""
    cfgs = [dict(samplerate=48000, mode="m"), dict(samplerate=48000, mode="s"), dict(samplerate=48000, mode="d"),
            dict(samplerate=24000, mode="s"), dict(samplerate=32000, mode="m"), dict(samplerate=16000, mode="s")]
    names = ["48k mono: overs at n = 0 and n = 1151 of frame 1; poisoned second row", "48k stereo: over in channel 1 only",
             "48k dual: overs at n = 18 l - 1 and 18 l; -32768 at unity", "24k stereo: idle, active, idle",
             "32k mono: one over", "16k stereo: at or below the ceiling throughout"]
    t = np.arange(nframes * N)
    bg = np.round(3000.0 * np.sin(2.0 * math.pi * 0.01 * t)).astype(np.int16)
    x = np.zeros((nframes, 6, 2, N), dtype=np.int16)
    for s in range(6):
        x[:, s, 0] = bg.reshape(nframes, N)
        x[:, s, 1] = -bg.reshape(nframes, N)
    x[:, 0, 1] = 0x5a5a                                              # a mono stream's second row: neither read nor written
    x[1, 0, 0, 0] = 32767; x[1, 0, 0, N - 1] = -32768
    x[1, 1, 1, 600] = 32767
    x[0, 2, 0, 18 * 7 - 1] = 32767; x[2, 2, 1, 18 * 33] = -32768; x[3, 2, 0, 900] = -32768; x[3, 2, 1, 901] = -32768
    x[1, 3, 0, 300:340] = 32767
    x[0, 4, 0, 1000] = 32767
    x[:, 5, 0] = np.round(20000.0 * np.sin(2.0 * math.pi * 0.013 * t)).reshape(nframes, N); x[:, 5, 1] = np.round(20000.0 * np.cos(2.0 * math.pi * 0.013 * t)).reshape(nframes, N)
    return cfgs, x, names


def structured():
    """the structured signals of the issue, each int16 [n] at 48 kHz: (name, samples)"""
    n = 4 * N
    t = np.arange(n)
    out = [("EBU Tech 3341 fs/4 sine at 45 degrees, full scale", TP.sine(0.25, math.pi / 4, math.sqrt(2.0), n, fade=480))]
    burst = np.concatenate([TP.sine(1000.0 / 48000.0, 0.0, 10.0 ** (-21.0 / 20.0), 2 * N), TP.sine(1000.0 / 48000.0, 0.0, 1.0, 2 * N)])
    out.append(("1 kHz burst from -21 dBFS to 0 dBFS", burst))
    out.append(("100 Hz full-scale sine", TP.sine(100.0 / 48000.0, 0.0, 1.0, n)))
    out.append(("full-scale period-14 square", np.where((t % 14) < 7, 32767, -32768).astype(np.int16)))
    f = 0.001 + (0.49 - 0.001) * t / n
    out.append(("sine sweep 0.001 .. 0.49 fs", np.clip(np.round(32767.0 * np.sin(2.0 * math.pi * np.cumsum(f))), -32768, 32767).astype(np.int16)))
    for period in (200, 97):
        gate = ((t // period) % 2) == 0
        out.append(("full-scale sine gated every %d" % period, np.where(gate, TP.sine(0.05, 0.0, 1.0, n), 0).astype(np.int16)))
        out.append(("Nyquist square gated every %d" % period, np.where(gate, np.where(t % 2 == 0, 32767, -32768), 0).astype(np.int16)))
    return out


def burst():
    """the structured burst alone"""
    return structured()[1][1]


CEILINGS = (300000000, 1 << 29, CEILING_DEFAULT, 1 << 30)


def random_signals(count=300, seed=2026):
    """-> list of (kind, int16 [2304], ceiling, S): noise, sparse clicks, random-sign squares, gated sines and random envelopes at four
    ceilings, S from a 16-sample release (2^30 / 16) to a second at 48 kHz (22369)"""
    rng = np.random.default_rng(seed)
    n = 2 * N
    t = np.arange(n)
    out = []
    for i in range(count):
        kind = ("noise", "clicks", "squares", "gated sine", "envelope")[i % 5]
        if kind == "noise":
            x = rng.integers(-32768, 32768, n)
        elif kind == "clicks":
            x = np.zeros(n, dtype=np.int64)
            at = rng.integers(0, n, rng.integers(1, 40))
            x[at] = rng.choice([-32768, 32767], len(at))
        elif kind == "squares":
            run = int(rng.integers(1, 9))
            x = np.repeat(rng.choice([-32768, 32767], n // run + 1), run)[:n]
        elif kind == "gated sine":
            period = int(rng.integers(20, 400))
            x = np.where(((t // period) % 2) == 0, np.round(32767.0 * np.sin(2.0 * math.pi * rng.uniform(0.01, 0.49) * t + rng.uniform(0, 6.28))), 0)
        else:
            env = np.interp(t, np.linspace(0, n, 12), rng.uniform(0.0, 1.0, 12))
            x = np.round(env * rng.integers(-32768, 32768, n))
        S = int(round(math.exp(rng.uniform(math.log(22369), math.log(U / 16)))))
        out.append((kind, np.clip(x, -32768, 32767).astype(np.int16), CEILINGS[(i // 5) % 4], S))
    return out


def one_stream(x):
    return TP.one_stream(x)
