"""Inputs shared by tests/test_minmax_forms_emu.py and tests/test_minmax_forms_gpu.py: the frame kernels' one-instruction maxima and minima
(csrc/tl_libm.h: tlm_max_gt, tlm_min_lt, tlm_maxabs_gt, tlm_maxabs2_gt, tlm_fmax_k) against the oracle, byte for byte.

A group is one batch of streams of 4 frames; every group of the issue's list has 8 streams, the single-stream cases ride in groups of their
own.  The oracle's bytes are computed once per process and never modified."""
import functools

import numpy as np

import oraclelib as O
from pcmgen import gen_pcm

NFRAMES = 4
# sites of the hook, in the order of csrc/tl_libm.h (TLM_MM_*)
SITES = ("scf", "jscf", "smr", "power", "bark", "cand", "xmax")


def _frames(x):
    """[2, NFRAMES * 1152] -> int16 [NFRAMES, 2, 1152]"""
    return np.ascontiguousarray(np.asarray(x).reshape(2, NFRAMES, 1152).transpose(1, 0, 2)).astype(np.int16)


def crafted():
    """eight streams: all zeros; full scale alternating +32767 / -32768 (both channels, and one channel a sample late); one impulse per frame
    (positive at sample 100, negative full scale at the frame's last sample); a tone at -90 dBFS (1 kHz, and 9.7 kHz against silence);
    zeros against the alternation"""
    n = NFRAMES * 1152
    t = np.arange(n)
    zero = np.zeros(n)
    alt = np.where(t & 1, -32768, 32767)
    imp = np.where(t % 1152 == 100, 32767, 0)
    imp_end = np.where(t % 1152 == 1151, -32768, 0)
    amp = 32768 * 10.0 ** (-90 / 20.0)                              # 1.04: the samples are -1, 0 and 1
    tone = np.rint(amp * np.sin(2 * np.pi * 1000.0 * t / 48000.0))
    tone_hi = np.rint(amp * np.sin(2 * np.pi * 9700.0 * t / 48000.0))
    assert np.abs(tone).max() == 1 and np.abs(tone_hi).max() == 1
    return [_frames(p) for p in ((zero, zero), (alt, alt), (alt, np.roll(alt, 1)), (imp, imp), (imp_end, imp), (tone, tone), (tone_hi, zero), (zero, alt))]


def generated():
    """eight streams of gen_pcm: tones + noise (four seeds), the stepped envelope, full-scale noise, channel-identical tones, +-1 LSB noise"""
    return [gen_pcm(20 + s, k, 0, NFRAMES) for s, k in enumerate((0, 0, 0, 0, 7, 4, 5, 6))]


@functools.lru_cache(maxsize=None)
def groups():
    """-> tuple of (name, cfg dict, tuple of pcm [NFRAMES, 2, 1152] per stream)"""
    g = []
    for psy in (1, 3):
        g.append(("48 kHz s 128 psy %d gen_pcm" % psy, dict(samplerate=48000, mode="s", kbps=128, psy=psy), tuple(generated())))
        g.append(("48 kHz s 128 psy %d crafted" % psy, dict(samplerate=48000, mode="s", kbps=128, psy=psy), tuple(crafted())))
        g.append(("48 kHz j 128 psy %d" % psy, dict(samplerate=48000, mode="j", kbps=128, psy=psy), tuple(generated()[:2] + crafted()[1:3])))
        g.append(("48 kHz m 64 psy %d mono pair" % psy, dict(samplerate=48000, mode="m", kbps=64, psy=psy), (gen_pcm(31, 0, 0, NFRAMES), gen_pcm(32, 7, 0, NFRAMES))))
        g.append(("44.1 kHz s 128 psy %d" % psy, dict(samplerate=44100, mode="s", kbps=128, psy=psy), (gen_pcm(33, 0, 0, NFRAMES),)))
        g.append(("32 kHz s 128 psy %d" % psy, dict(samplerate=32000, mode="s", kbps=128, psy=psy), (gen_pcm(34, 0, 0, NFRAMES),)))
    g.append(("48 kHz s 128 psy 0", dict(samplerate=48000, mode="s", kbps=128, psy=0), (gen_pcm(35, 0, 0, NFRAMES),)))
    return tuple(g)


@functools.lru_cache(maxsize=None)
def oracle_bytes(gi):
    """the oracle's stream (every frame and the flushed one) of each stream of group gi"""
    _, cfg, pcms = groups()[gi]
    return tuple(O.oracle_stream(p, **cfg)[0] for p in pcms)
