"""Streams, configurations and a numpy restatement of the filterbank's operand table for tests/test_fb_fold_emu.py and
tests/test_fb_fold_gpu.py.

csrc/mp2_fb.h adds the two window sums of a yprime in every lane alike; the minus of yprime[i] = y[i+16] - y[80-i] (i >= 17) and the
missing second term of yprime[0] = y[16] are in TlTables::enwindow_s (csrc/mp2_host.cpp): window / 32768 with rows (index mod 64) 49..63
negated and row 48, which no yprime uses, +0.0.  Where that could differ from the subtraction is the sign of a zero, so the signals
here make most window sums exact zeros or single products: silence, DC, lone impulses, and combs that are non-zero only where
n = r (mod 64) for the rows the fold touches (48, 49, 63), their neighbours (47, 0, 15, 17) and row 16."""
import functools

import numpy as np

import oraclelib as O
from pcmgen import gen_pcm

NFRAMES = 3
COMB_ROWS = (0, 15, 16, 17, 47, 48, 49, 63)

# (name, configuration as tests/emulib.py takes it); the last one runs as mono streams of one configuration, which share waves in pairs
CONFIGS = [
    ("s128_psy1", dict(samplerate=48000, mode="s", kbps=128, psy=1)),
    ("j128_psy1", dict(samplerate=48000, mode="j", kbps=128, psy=1)),
    ("s128_psy3", dict(samplerate=48000, mode="s", kbps=128, psy=3)),
    ("d128_psy0", dict(samplerate=48000, mode="d", kbps=128, psy=0)),
    ("m64_32k_psy1", dict(samplerate=32000, mode="m", kbps=64, psy=1)),
]


def _both(x):
    """one channel's samples [NFRAMES * 1152] -> int16 [NFRAMES, 2, 1152], the same in both channels"""
    x = np.asarray(x, dtype=np.int64).reshape(NFRAMES, 1, 1152)
    assert x.min() >= -32768 and x.max() <= 32767
    return np.ascontiguousarray(np.repeat(x, 2, axis=1)).astype(np.int16)


@functools.lru_cache(maxsize=None)
def signals():
    """-> tuple of (name, int16 [NFRAMES, 2, 1152])"""
    n = NFRAMES * 1152
    out = [("silence", _both(np.zeros(n)))]
    for v in (-1, -32768, 32767):
        out.append(("dc%+d" % v, _both(np.full(n, v))))
    imp = np.zeros(n)
    for f in range(NFRAMES):                                   # one impulse of +1 and one of -1 per frame, at odd distances
        imp[1152 * f + 101 + 37 * f] = 1
        imp[1152 * f + 700 + 53 * f] = -1
    out.append(("impulses", _both(imp)))
    taps = np.arange(n // 64)
    for r in COMB_ROWS:
        for v in (1, 32767):
            for pat, sign in (("plus", np.ones(taps.size)), ("minus", -np.ones(taps.size)), ("alt", 1.0 - 2.0 * (taps & 1))):
                x = np.zeros(n)
                x[r::64] = v * sign
                out.append(("comb_r%d_%s_%d" % (r, pat, v), _both(x)))
    out.append(("tones_noise", gen_pcm(41, 0, 0, NFRAMES)))
    return tuple(out)


def batch_pcm():
    """every signal as a stream of one batch: int16 [NFRAMES, nsignals, 2, 1152]"""
    return np.ascontiguousarray(np.stack([p for _, p in signals()], axis=1))


@functools.lru_cache(maxsize=None)
def oracle(cfg_name):
    """per signal of the configuration: (all bytes with the finish, taps of every frame as a list of dicts)"""
    cfg = dict(CONFIGS)[cfg_name]
    res = []
    for _, pcm in signals():
        e = O.OracleEncoder(**cfg)
        chunks, taps = [], []
        for f in pcm:
            chunks.append(e.encode(f))
            taps.append(e.taps())
        chunks.append(e.finish())
        e.close()
        res.append((b"".join(chunks), taps))
    return res


def check_against_oracle(cfg_name, got, tail, taps):
    """bytes (encode + flush) per stream and the taps array [NFRAMES, nsignals] of a batch of batch_pcm() against the oracle:
    sb_sample as raw 64-bit words, scalar, bit_alloc, scfsi, and the frame bytes.  -> number of compared sb_sample words that are zeros"""
    nch = 1 if dict(CONFIGS)[cfg_name]["mode"] == "m" else 2
    zeros = 0
    for s, ((name, _), (ref, rtaps)) in enumerate(zip(signals(), oracle(cfg_name))):
        for f in range(NFRAMES):
            t, r = taps[f, s], rtaps[f]
            a = np.ascontiguousarray(t["sb_sample"][:nch]).view(np.uint64)
            b = np.ascontiguousarray(r["sb_sample"][:nch]).view(np.uint64)
            bad = np.argwhere(a != b)
            assert bad.size == 0, (cfg_name, name, f, "sb_sample [ch, granule, block, sb]", bad[:4].tolist(),
                                   [hex(int(a[tuple(i)])) for i in bad[:4]], [hex(int(b[tuple(i)])) for i in bad[:4]])
            zeros += int(np.count_nonzero((b << np.uint64(1)) == 0))
            for k in ("scalar", "bit_alloc", "scfsi"):
                assert np.array_equal(t[k][:nch], r[k][:nch]), (cfg_name, name, f, k)
        assert got[s] + tail[s] == ref, (cfg_name, name, "frame bytes")
    return zeros


def folded_table(enwindow):
    """TlTables::enwindow_s restated from the window: / 32768, rows 49..63 negated, row 48 +0.0"""
    w = np.asarray(enwindow, dtype=np.float64)
    assert w.shape == (512,)
    t = w / 32768.0
    row = np.arange(512) & 63
    t[row > 48] = -t[row > 48]
    t[row == 48] = 0.0
    return t
