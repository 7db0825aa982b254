"""Support for the compare monitor tests (test_compare_emu.py, test_compare_gpu.py): the rule of include/toolame_batch.h (tlb_compare_device)
as a plain numpy / Python-int loop -- the oracle, nothing else -- the emulation of the kernel (tests/emu/mp2_compare_emu.cpp, compiled into
a temporary directory), and the inputs and stream sets the two test files share."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from declib import BAD_MASK, EMPTY, REPORT_DTYPE
from pcmgen import gen_pcm

ROOT = Path(__file__).resolve().parent.parent
DELAY = 481
N = 1152
RECORD_DTYPE = np.dtype([("sxx", np.int64, (2,)), ("syy", np.int64, (2,)), ("sxy", np.int64, (2,)), ("sxz", np.int64, (2,)),
                         ("frames_compared", np.uint32), ("frames_judged", np.uint32), ("mismatch_frames", np.uint32), ("mismatch_run", np.uint32),
                         ("swapped_frames", np.uint32), ("last_flags", np.uint32), ("reserved_", np.uint32, (2,))])
COUNTERS = ("frames_compared", "frames_judged", "mismatch_frames", "mismatch_run", "swapped_frames", "last_flags")
JUDGED0, JUDGED1, MISMATCH, SWAPPED, SKIPPED = (1 << i for i in range(5))
# what every test passes: a frame at 256 LSB rms is loud enough to judge, and half the energy must correlate
PARAMS = (N * 256 * 256, 1, 2)
# six streams: stereo, joint stereo, dual channel, a mono pair (two streams of one configuration next to each other share a wave in the
# encoder) and an LSF stream
STREAMS = [dict(samplerate=48000, mode="s", kbps=192), dict(samplerate=48000, mode="j", kbps=128), dict(samplerate=48000, mode="d", kbps=128),
           dict(samplerate=48000, mode="m", kbps=96), dict(samplerate=48000, mode="m", kbps=96), dict(samplerate=24000, mode="m", kbps=64)]


def nch_of(cfg):
    return 1 if cfg["mode"] == "m" else 2


def noise(nframes, nstreams, seed=1000):
    """Noise-based programme at about quarter scale, an independent seed per stream (pcmgen keys the channel itself): the full-scale noise
    of pcmgen (kind 4) under a 7-tap triangle (1 2 3 4 3 2 1) / 16, which runs across the frame borders.  rms 7.8 k of 32 k; most of the
    energy lies below a quarter of the sample rate, where every configuration of the tests transmits its subbands, so that the codec's
    own error stays small beside the faults the tests inject.  Integers only.  -> int16 [nframes][nstreams][2][1152]"""
    out = np.zeros((nframes, nstreams, 2, N), dtype=np.int16)
    tri = np.array([1, 2, 3, 4, 3, 2, 1], dtype=np.int64)
    for s in range(nstreams):
        raw = gen_pcm(seed=seed + 17 * s, kind=4, frame=0, nframes=nframes).astype(np.int64)
        for c in range(2):
            v = np.convolve(raw[:, c].reshape(-1), tri)[:nframes * N] >> 4
            out[:, s, c] = v.reshape(nframes, N).astype(np.int16)
    return out


def white(nframes, nstreams, seed=500):
    """white noise at quarter scale (the delay measurement) -> int16 [nframes][nstreams][2][1152]"""
    return np.stack([gen_pcm(seed=seed + 17 * s, kind=4, frame=0, nframes=nframes) >> 2 for s in range(nstreams)], axis=1).astype(np.int16)


def mispaired_sums(pcm, dec, nch):
    """stream k's decoded audio against stream k + 1's input at the delay, for the slots whose history is a whole frame (f >= 2) and the
    channels both streams have -> [(sxy, sxx, syy)] in Python ints"""
    nf, ns = dec.shape[:2]
    out = []
    for k in range(ns - 1):
        for c in range(min(nch[k], nch[k + 1])):
            x = pcm[:, k + 1, c].reshape(-1).astype(np.int64)
            for f in range(2, nf):
                xs, y = x[(f - 1) * N - DELAY:f * N - DELAY], dec[f, k, c].astype(np.int64)
                out.append((int((xs * y).sum()), int((xs * xs).sum()), int((y * y).sum())))
    return out


def planar_of(inter, nch):
    """a tick's interleaved input int16 [ns][2304] -> planar [1][ns][2][1152] as ingest hands it to the encoder at 0 dB gain (a one-channel
    stream is its first 1152 values; its channel 1 is never looked at)"""
    ns = inter.shape[0]
    out = np.zeros((1, ns, 2, N), dtype=np.int16)
    for s in range(ns):
        if nch[s] == 2:
            out[0, s] = inter[s].reshape(N, 2).T
        else:
            out[0, s, 0] = inter[s, :N]
    return out


def interleaved_of(pcm, nch):
    """planar [nf][ns][2][1152] -> the ticks' interleaved input [nf][ns][2304]"""
    nf, ns = pcm.shape[:2]
    out = np.zeros((nf, ns, 2 * N), dtype=np.int16)
    for s in range(ns):
        if nch[s] == 2:
            out[:, s] = pcm[:, s].transpose(0, 2, 1).reshape(nf, 2 * N)
        else:
            out[:, s, :N] = pcm[:, s, 0]
            out[:, s, N:] = 0x1234                                   # never read
    return out


def match(sab, saa, sbb, num, den):
    return sab > 0 and den * den * sab * sab >= num * num * saa * sbb


def corr(sab, saa, sbb):
    return sab / float(np.sqrt(float(saa) * float(sbb))) if saa > 0 and sbb > 0 else 0.0


class Oracle:
    """the definitions, slot by slot, one stream at a time; keeps the history (previous input frame + the D samples before it) itself"""

    def __init__(self, nch):
        self.nch = list(nch)
        self.hist = np.zeros((len(self.nch), 2, DELAY + N), dtype=np.int64)

    def reset(self, s=-1):
        if s < 0:
            self.hist[:] = 0
        else:
            self.hist[s] = 0

    def compare(self, in_pcm, dec_pcm, status, params, record=None):
        """in_pcm [nf][ns][2][1152] or None (the flush: nf == 1, no advance), dec_pcm the same shape, status ints [nf][ns]; record to go on
        from (not changed) or None -> (new RECORD_DTYPE [ns], list of the sums of every compared slot: (f, s, sxx, syy, sxy, sxz))"""
        status = np.asarray(status)
        nf, ns = status.shape
        assert in_pcm is not None or nf == 1
        emin, num, den = (int(v) for v in params)
        out = np.zeros(ns, dtype=RECORD_DTYPE) if record is None else record.copy()
        seen = []
        for s in range(ns):
            r = {k: int(out[s][k]) for k in COUNTERS}
            sums = {k: [int(v) for v in out[s][k]] for k in ("sxx", "syy", "sxy", "sxz")}
            for f in range(nf):
                if int(status[f, s]) & (EMPTY | BAD_MASK):
                    r["last_flags"] = SKIPPED
                else:
                    x = [[int(v) for v in self.hist[s, c, :N]] for c in range(2)]
                    y = [[int(v) for v in dec_pcm[f, s, c]] for c in range(2)]
                    cs = range(self.nch[s])
                    sxx, syy, sxy, sxz = [0, 0], [0, 0], [0, 0], [0, 0]
                    for c in cs:
                        sxx[c] = sum(a * a for a in x[c])
                        syy[c] = sum(b * b for b in y[c])
                        sxy[c] = sum(a * b for a, b in zip(x[c], y[c]))
                        if self.nch[s] == 2:
                            sxz[c] = sum(a * b for a, b in zip(x[c], y[1 - c]))
                    sums = dict(sxx=sxx, syy=syy, sxy=sxy, sxz=sxz)
                    seen.append((f, s, sxx, syy, sxy, sxz))
                    judged = [c in cs and sxx[c] >= emin for c in range(2)]
                    ok = [judged[c] and match(sxy[c], sxx[c], syy[c], num, den) for c in range(2)]
                    mismatch = any(judged[c] and not ok[c] for c in range(2))
                    swapped = (self.nch[s] == 2 and all(judged) and not any(ok)
                               and all(match(sxz[c], sxx[c], syy[1 - c], num, den) for c in range(2)))
                    r["frames_compared"] += 1
                    if any(judged):
                        r["frames_judged"] += 1
                        if mismatch:
                            r["mismatch_frames"] += 1
                            r["mismatch_run"] += 1
                        else:
                            r["mismatch_run"] = 0
                    if swapped:
                        r["swapped_frames"] += 1
                    r["last_flags"] = (JUDGED0 if judged[0] else 0) | (JUDGED1 if judged[1] else 0) | (MISMATCH if mismatch else 0) | (SWAPPED if swapped else 0)
                if in_pcm is not None:
                    for c in range(self.nch[s]):
                        self.hist[s, c] = np.concatenate([self.hist[s, c, N:], np.asarray(in_pcm[f, s, c], dtype=np.int64)])
            for k in COUNTERS:
                out[s][k] = r[k]
            for k in ("sxx", "syy", "sxy", "sxz"):
                out[s][k] = sums[k]
        return out, seen


def same(got, want, what=""):
    assert got.dtype == RECORD_DTYPE == want.dtype
    for k in RECORD_DTYPE.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert got.tobytes() == want.tobytes(), what


def build_emu(outdir):
    """tests/emu/mp2_compare_emu.cpp -> outdir/libmp2compareemu.so (the flags of tests/emu/Makefile)"""
    so = Path(outdir) / "libmp2compareemu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function",
                    "-Wno-unused-variable", "-Wno-unknown-pragmas", "-Wno-unused-but-set-variable", "-Wno-maybe-uninitialized", "-shared", "-o", str(so),
                    str(ROOT / "tests" / "emu" / "mp2_compare_emu.cpp"), "-lm"], check=True)
    return so


class CompareEmu:
    """N streams on the emulated compare kernel; compare() mirrors tlb_compare_host, the history lives here as the batch's lives on the device"""

    def __init__(self, so, nch):
        L = self.L = C.CDLL(str(so))
        L.cmp_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        assert L.cmp_sizeof_record() == RECORD_DTYPE.itemsize == 96 and L.cmp_delay() == DELAY
        self.nch = np.ascontiguousarray(nch, dtype=np.int32)
        self.hist = np.zeros((len(self.nch), 2, L.cmp_hist_samples()), dtype=np.int16)

    def reset(self, s=-1):
        if s < 0:
            self.hist[:] = 0
        else:
            self.hist[s] = 0

    def compare(self, in_pcm, dec_pcm, report, params, record=None):
        rep = np.ascontiguousarray(report, dtype=REPORT_DTYPE)
        nf, ns = rep.shape
        dec = np.ascontiguousarray(dec_pcm, dtype=np.int16)
        inp = None if in_pcm is None else np.ascontiguousarray(in_pcm, dtype=np.int16)
        assert dec.shape == (nf, ns, 2, N) and (inp is None or inp.shape == dec.shape) and ns == len(self.nch)
        if record is None:
            record = np.zeros(ns, dtype=RECORD_DTYPE)
        assert record.dtype == RECORD_DTYPE and record.shape == (ns,) and record.flags.c_contiguous
        rc = self.L.cmp_compare(None if inp is None else inp.ctypes.data, dec.ctypes.data, rep.ctypes.data, nf, ns, self.nch.ctypes.data,
                                int(params[0]), int(params[1]), int(params[2]), self.hist.ctypes.data, record.ctypes.data)
        assert rc == 0, rc
        return record


def reports_of(status):
    rep = np.zeros(np.asarray(status).shape, dtype=REPORT_DTYPE)
    rep["status"] = np.asarray(status, dtype=np.uint32)
    return rep


def check_input_conditions(seen, mispaired, loud):
    """The conditions the issue sets on the test inputs, asserted on the ORACLE's sums so that a threshold near the edge cannot make a test
    vacuous.  seen: the oracle's sums of an undisturbed run, restricted by the caller to frames whose history holds a whole input frame;
    mispaired: (sab, saa, sbb) triples of stream k's decode against stream k + 1's input; loud: set of loud streams."""
    n = 0
    for f, s, sxx, syy, sxy, sxz in seen:
        if s not in loud:
            continue
        for c in range(2):
            if sxx[c] == 0 and c == 1:
                continue                                             # a one-channel stream
            assert sxx[c] >= PARAMS[0], ("a loud stream's frame is not judged", f, s, c, sxx[c])
            assert corr(sxy[c], sxx[c], syy[c]) >= 0.75, ("healthy correlation below 3/4", f, s, c, corr(sxy[c], sxx[c], syy[c]))
            n += 1
    for sab, saa, sbb in mispaired:
        assert abs(corr(sab, saa, sbb)) <= 0.25, ("mispaired correlation above 1/4", corr(sab, saa, sbb))
    assert n > 0 and len(mispaired) > 0
