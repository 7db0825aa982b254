"""Inputs shared by tests/test_thr_min_emu.py and tests/test_thr_min_gpu.py: the threshold stage of psy models 1 and 3 (csrc/mp2_psy13.h)
with the subband minimum of psy 1 as one v_min_f64 per row (csrc/tl_libm.h: tlm_min_rows_lt) and without the order test on the paired
path of tl_psy1_stereo, against the oracle (psy 3 shares the stage's helpers and rides along).

64 streams of 2 frames in ONE mixed batch: psy 1 and psy 3; stereo, joint stereo and pairs of mono streams; 48, 44.1 and 32 kHz; silence,
a full-scale alternation, lone impulses, a tone at -90 dBFS, the eight kinds of pcmgen, and the tone-labelling stress signals of
tests/test_psy1_pairing.py, two of which have a dead head (the order in which the masker lists are NOT ascending by construction) and
one of which (the comb) has tone lists too long for the paired pass.  The oracle's results are computed once per process and never
modified."""
import functools

import numpy as np

import oraclelib as O
from pcmgen import gen_pcm
from test_psy1_pairing import DEAD_HEAD_CH0, DEAD_HEAD_CH1, crafted as stress
from test_psy1_pairing_back import comb

NFRAMES = 2


def _frames(l, r):
    """two channels of NFRAMES * 1152 samples -> int16 [NFRAMES, 2, 1152]"""
    return np.ascontiguousarray(np.stack([l, r]).reshape(2, NFRAMES, 1152).transpose(1, 0, 2)).astype(np.int16)


def crafted():
    """name -> pcm: all zeros; full scale alternating +32767 / -32768; one impulse per frame (positive at sample 100; negative full scale at
    the frame's last sample in channel 0 against the first in channel 1); a 1 kHz tone at -90 dBFS (samples -1, 0, 1)"""
    n = NFRAMES * 1152
    t = np.arange(n)
    zero = np.zeros(n)
    alt = np.where(t & 1, -32768, 32767)
    imp = np.where(t % 1152 == 100, 32767, 0)
    imp_end = np.where(t % 1152 == 1151, -32768, 0)
    tone = np.rint(32768 * 10.0 ** (-90 / 20.0) * np.sin(2 * np.pi * 1000.0 * t / 48000.0))
    assert np.abs(tone).max() == 1
    return dict(silence=_frames(zero, zero), alternation=_frames(alt, np.roll(alt, 1)), impulse=_frames(imp, imp),
                impulse_end=_frames(imp_end, imp), tone90=_frames(tone, zero))


def _kind(k, seed):
    return gen_pcm(seed, k, 0, NFRAMES)


@functools.lru_cache(maxsize=None)
def streams():
    """-> tuple of (name, cfg dict, pcm [NFRAMES, 2, 1152]); 64 entries.  The two streams of a mono pair are neighbours."""
    c = crafted()
    s = []
    for psy in (1, 3):
        st = dict(samplerate=48000, mode="s", kbps=128, psy=psy)
        s += [("kind%d" % k, st, _kind(k, 40 + k)) for k in range(8)]
        s += [(name, st, c[name]) for name in ("silence", "alternation", "impulse", "impulse_end", "tone90")]
        jt = dict(samplerate=48000, mode="j", kbps=128, psy=psy)
        s += [("kind0", jt, _kind(0, 50)), ("kind7", jt, _kind(7, 51)), ("alternation", jt, c["alternation"])]
        mo = dict(samplerate=48000, mode="m", kbps=64, psy=psy)
        s += [("kind0", mo, _kind(0, 52)), ("kind7", mo, _kind(7, 53))]
        for fs, other in ((44100, "silence"), (32000, "tone90")):
            s += [("kind0", dict(samplerate=fs, mode="s", kbps=128, psy=psy), _kind(0, 54)),
                  (other, dict(samplerate=fs, mode="s", kbps=128, psy=psy), c[other]),
                  ("kind3", dict(samplerate=fs, mode="j", kbps=128, psy=psy), _kind(3, 55))]
        s += [("kind4", dict(samplerate=32000, mode="s", kbps=128, psy=psy), _kind(4, 56)),
              ("kind5", dict(samplerate=32000, mode="s", kbps=128, psy=psy), _kind(5, 57))]
        s += [("stress%d" % seed, st, stress(seed)[:NFRAMES]) for seed in (DEAD_HEAD_CH0, 0)]
    st = dict(samplerate=48000, mode="s", kbps=128, psy=1)
    s += [("stress%d" % seed, st, stress(seed)[:NFRAMES]) for seed in (DEAD_HEAD_CH1, 2, 4)] + [("comb0", st, comb(0)[:NFRAMES])]
    for fs in (44100, 32000):
        mo = dict(samplerate=fs, mode="m", kbps=64, psy=1)
        s += [("kind0", mo, _kind(0, 58)), ("kind6", mo, _kind(6, 59))]
    assert len(s) == 64, len(s)
    return tuple(("%d %s %d psy %d %s" % (cfg["samplerate"], cfg["mode"], cfg["kbps"], cfg["psy"], name), cfg, pcm) for name, cfg, pcm in s)


@functools.lru_cache(maxsize=None)
def oracle():
    """per stream: (the oracle's bytes, every frame and the flushed one; its SMR taps [NFRAMES, 2, 32]; nch; entries of an SMR row that the
    model writes: sblimit for psy 1, 32 for psy 3)"""
    res = []
    for _, cfg, pcm in streams():
        e = O.OracleEncoder(**cfg)
        chunks, smr = [], []
        for f in range(NFRAMES):
            chunks.append(e.encode(pcm[f]))
            smr.append(e.taps()["smr"])
        chunks.append(e.finish())
        res.append((b"".join(chunks), np.stack(smr), e.nch, e.sblimit if cfg["psy"] == 1 else 32))
        e.close()
    return tuple(res)


@functools.lru_cache(maxsize=None)
def flagship():
    """8 streams x 4 frames of the benchmark's flagship shape (48 kHz, 's', 128 kbps, psy 1) -> (cfg, pcm [4, 8, 2, 1152], oracle bytes)"""
    cfg = dict(samplerate=48000, mode="s", kbps=128, psy=1)
    pcms = [gen_pcm(70 + s, (0, 0, 0, 0, 7, 4, 5, 6)[s], 0, 4) for s in range(8)]
    return cfg, np.stack(pcms, axis=1), tuple(O.oracle_stream(p, **cfg)[0] for p in pcms)
