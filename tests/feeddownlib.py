"""Support for the down-feed tests (test_feed_down_*.py): the schedule's closed form in Python ints, the numpy oracle -- feedlib's decode of the
WANTED frames, the channel map, decimatelib's formula, cut into ticks; it shares no code with the emulation --, the emulation of the kernels
(tests/emu/mp2_feed_down_emu.cpp, compiled into a temporary directory), its sanitizer driver (tests/emu/mp2_feed_down_san_main.cpp, a program
of its own), and the stream set and inputs the test files share.  A plain module: nothing here is collected by pytest."""
import ctypes as C
import os
import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import decimatelib as DC
import declib as D
import feedlib as F

ROOT = F.ROOT
N = 1152
ES = 24000
POISON = F.POISON
REPORT_DTYPE = F.REPORT_DTYPE
EMPTY = D.EMPTY
UNWANTED = 0x100
RATIOS = DC.RATIOS                                                   # feed rate -> (L, M)
NTICKS = 8                                                           # 80/147: past the first one-frame tick (6) and the five-tick need cycle; two periods of 3/4
CUTS = ((8,), (1, 3, 4), (1,) * 8)
# the stream set: feed (rate, mode of the source encoder, kbps, pcmgen kind) or None, the stream's mode (its rate is 24 kHz)
STREAMS = [dict(feed=(48000, "s", 192, 0), mode="s"),
           dict(feed=(48000, "s", 128, 3), mode="m"),                # map
           dict(feed=(44100, "s", 128, 5), mode="s"),                # both frame lengths occur (padding slots)
           dict(feed=(32000, "m", 64, 4), mode="s"),                 # one to two
           dict(feed=(32000, "s", 128, 7), mode="m"),
           dict(feed=(48000, "m", 64, 2), mode="m"),
           dict(feed=None, mode="s")]                                # a stream without a feed


def S(f, L, M):
    """source frames consumed before tick f: ceil(1152 f M / L)"""
    return -((-N * f * M) // L)


def K(f, L, M):
    """feed frames that must have arrived by tick f; K(-1) = 0"""
    return -(-S(f + 1, L, M) // N) if f >= 0 else 0


def want(f, L, M):
    return K(f, L, M) - K(f - 1, L, M)


def fcfg_of(st):
    return F.feed_cfg_of(st["feed"]) if st["feed"] else None


def enc_nch(st):
    return 1 if st["mode"] == "m" else 2


def lm_of(st):
    return RATIOS[st["feed"][0]]


_frames = {}


def feed_frames(i, st, n):
    """the oracle encoder's first `n` frames of stream i's feed (CPU), once per process and length"""
    key = (i, st["feed"], n)
    if key not in _frames:
        _frames[key] = F.oracle_frames(st["feed"], F.case_pcm(60 + i, st["feed"], n))
    return _frames[key]


def slots_of(fr, L, M, nticks):
    """the frames `fr` on the schedule: per tick two (bytes, len), the next one or two frames as want says, an empty slot 1 otherwise"""
    sl, k = [], 0
    for f in range(nticks):
        w = want(f, L, M)
        sl.append([(fr[k + j], len(fr[k + j])) if j < w else (b"", 0) for j in range(2)])
        k += w
    assert k == len(fr)
    return sl


def slots_on_schedule(streams, nticks=NTICKS):
    """per stream a list per tick of two (bytes, len): the next one or two feed frames as want says, empty slots otherwise (and for a stream
    without a feed) -> (slot lists, per stream the frames in wanted order)"""
    lists, used = [], []
    for i, st in enumerate(streams):
        if not st["feed"]:
            lists.append([[(b"", 0), (b"", 0)] for _ in range(nticks)]); used.append([])
            continue
        L, M = lm_of(st)
        fr = feed_frames(i, st, K(nticks - 1, L, M))
        lists.append(slots_of(fr, L, M, nticks)); used.append(list(fr))
    return lists, used


def slots_to_arrays(lists, stride):
    """per stream, per tick two (bytes, len) -> frames uint8 [nticks][ns][2][stride], lens int32 [nticks][ns][2]; a length may lie (hostile
    input): the bytes are cut to the stride"""
    nt, ns = len(lists[0]), len(lists)
    frames = np.zeros((nt, ns, 2, stride), dtype=np.uint8)
    lens = np.zeros((nt, ns, 2), dtype=np.int32)
    for s, sl in enumerate(lists):
        for f, pair in enumerate(sl):
            for j, (b, n) in enumerate(pair):
                b = bytes(b)[:stride]
                frames[f, s, j, :len(b)] = np.frombuffer(b, dtype=np.uint8)
                lens[f, s, j] = n
    return frames, lens


def channel_map(x, fch, sch):
    """x int [n][fch] -> [n][the decimator's channels]: two to one is (L + R + 1) >> 1; one to two stays one (the OUTPUT goes to both)"""
    x = np.asarray(x, dtype=np.int64)
    if fch == 2 and sch == 1:
        return ((x[:, 0] + x[:, 1] + 1) >> 1)[:, None]
    return x


def oracle_ticks(x, fs, fch, sch, nticks):
    """x int [source frames since the reset][fch] -> int16 [nticks][2304] as the ingest reads it (zeros where nothing is written)"""
    y = DC.oracle_stream(channel_map(x, fch, sch), fs, ES, N * nticks)
    if fch == 1 and sch == 2:
        y = np.repeat(y, 2, axis=1)
    out = np.zeros((nticks, 2 * N), dtype=np.int16)
    out[:, :N * sch] = y.astype(np.int16).reshape(nticks, N * sch)
    return out


def oracle_pcm(frames, st, nticks=NTICKS):
    """frames: the stream's WANTED frames in order (bytes, or None for one that decodes to silence) -> int16 [nticks][2304]"""
    fc = fcfg_of(st)
    fch = fc["channels"]
    d = F.numpy_feed_pcm(frames, fc)[:, :N * fch].reshape(-1, fch)
    return oracle_ticks(d, st["feed"][0], fch, enc_nch(st), nticks)


def written(streams, nticks):
    """bool [nticks][ns][2304]: what a down-feed call writes: the first 1152 * channels of the STREAM where it has a down feed"""
    m = np.zeros((nticks, len(streams), 2 * N), dtype=bool)
    for s, st in enumerate(streams):
        if st["feed"]:
            m[:, s, :N * enc_nch(st)] = True
    return m


def expected_status(streams, lens):
    """-> (wanted bool [nt][ns][2], status uint32 [nt][ns][2] of every slot that is NOT wanted) for ticks counted from a reset"""
    nt, ns = lens.shape[:2]
    w = np.zeros((nt, ns, 2), dtype=bool)
    st_ = np.full((nt, ns, 2), EMPTY, dtype=np.uint32)
    for s, st in enumerate(streams):
        if not st["feed"]:
            continue
        L, M = lm_of(st)
        for f in range(nt):
            w[f, s, :want(f, L, M)] = True
    st_[(lens > 0) & ~w & np.array([bool(st["feed"]) for st in streams])[None, :, None]] |= UNWANTED
    return w, st_


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation and its sanitizer driver
_FLAGS = F._FLAGS
_SRC = [str(ROOT / "tests" / "emu" / "mp2_feed_down_emu.cpp"), str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp")]
_built = {}


def build_emu():
    """tests/emu/mp2_feed_down_emu.cpp + csrc/mp2_host.cpp -> a temporary directory, once per process"""
    if "so" not in _built:
        so = Path(tempfile.mkdtemp(prefix="fdemu")) / "libmp2feeddownemu.so"
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + _FLAGS + ["-o", str(so)] + _SRC + ["-lm"], check=True)
        _built["so"] = so
    return _built["so"]


def build_san_driver():
    """tests/emu/mp2_feed_down_san_main.cpp + the emulation + csrc/mp2_host.cpp as ONE program under AddressSanitizer + UBSan (linked, not preloaded)"""
    if "san" not in _built:
        exe = Path(tempfile.mkdtemp(prefix="fdsan")) / "mp2_feed_down_san"
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + _FLAGS + ["-o", str(exe),
                        str(ROOT / "tests" / "emu" / "mp2_feed_down_san_main.cpp")] + _SRC + ["-lm"], check=True)
        _built["san"] = exe
    return _built["san"]


def rows_of(streams):
    return [(fcfg_of(st), ES, enc_nch(st)) for st in streams]


def run_san_driver(exe, workdir, streams, cases):
    """cases: [[(frames, lens), ...]]: per case the calls of one run from the reset -> per case (report [nt][ns][2], pcm [nt][ns][2304]) over all
    its ticks, as the sanitized program wrote them (every sample POISON before each call)"""
    rows = rows_of(streams)
    fin, fout = Path(workdir) / "cases.bin", Path(workdir) / "results.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ii", len(rows), len(cases)))
        for c, rate, nch in rows:
            f.write(struct.pack("<qiiqi", c["samplerate"] if c else 0, c["bitrate"] if c else 0, c["channels"] if c else 0, rate, nch))
        for calls in cases:
            f.write(struct.pack("<i", len(calls)))
            for fr, ln in calls:
                f.write(struct.pack("<i", fr.shape[0]))
                f.write(np.ascontiguousarray(fr, dtype=np.uint8).tobytes())
                f.write(np.ascontiguousarray(ln, dtype=np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    blob, pos, out = fout.read_bytes(), 0, []
    for calls in cases:
        reps, pcms = [], []
        for fr, _ in calls:
            nf, ns = fr.shape[0], fr.shape[1]
            n = REPORT_DTYPE.itemsize * nf * ns * 2
            reps.append(np.frombuffer(blob[pos:pos + n], dtype=REPORT_DTYPE).reshape(nf, ns, 2)); pos += n
            n = 2 * nf * ns * 2304
            pcms.append(np.frombuffer(blob[pos:pos + n], dtype=np.int16).reshape(nf, ns, 2304)); pos += n
        out.append((np.concatenate(reps), np.concatenate(pcms)))
    assert pos == len(blob)
    return out


class FeedDownEmu:
    """a stream set on the emulated down-feed path; decode() mirrors tlb_feed_down_host with an output buffer that holds POISON"""

    def __init__(self, streams):
        L = self.L = C.CDLL(str(build_emu()))
        L.fd_create.restype = C.c_void_p
        L.fd_create.argtypes = [C.c_int] + [C.c_void_p] * 6
        L.fd_destroy.argtypes = [C.c_void_p]
        L.fd_stride.argtypes = [C.c_void_p]
        L.fd_reset.argtypes = [C.c_void_p, C.c_int]
        L.fd_pos.argtypes = [C.c_void_p, C.c_int]
        L.fd_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert L.fd_sizeof_report() == REPORT_DTYPE.itemsize
        rows = rows_of(streams)
        n = self.n = len(rows)
        fs = (C.c_long * n)(*[c["samplerate"] if c else 0 for c, _, _ in rows])
        kb = (C.c_int * n)(*[c["bitrate"] if c else 0 for c, _, _ in rows])
        ch = (C.c_int * n)(*[c["channels"] if c else 0 for c, _, _ in rows])
        er = (C.c_long * n)(*[r for _, r, _ in rows])
        en = (C.c_int * n)(*[k for _, _, k in rows])
        err = C.c_int(0)
        self.h = L.fd_create(n, fs, kb, ch, er, en, C.byref(err))
        assert self.h, err.value
        self.stride = L.fd_stride(self.h)

    def decode(self, frames, lens, init=None):
        """init: what the output buffer holds before the call (None: POISON everywhere) -> (pcm [nf][ns][2304], report [nf][ns][2])"""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        assert frames.shape == (nf, self.n, 2, self.stride)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        assert ln.shape == (nf, self.n, 2)
        rep = np.zeros((nf, self.n, 2), dtype=REPORT_DTYPE)
        pcm = np.full((nf, self.n, 2304), POISON, dtype=np.int16) if init is None else np.array(init, dtype=np.int16, order="C", copy=True)
        rc = self.L.fd_decode(self.h, frames.ctypes.data, ln.ctypes.data, nf, pcm.ctypes.data, rep.ctypes.data)
        assert rc == 0, rc
        return pcm, rep

    def run_cuts(self, frames, lens, cuts):
        """the ticks of (frames, lens) call by call -> (pcm, report) over all of them"""
        out, f0 = [], 0
        for n in cuts:
            out.append(self.decode(frames[f0:f0 + n], lens[f0:f0 + n]))
            f0 += n
        return np.concatenate([p for p, _ in out]), np.concatenate([r for _, r in out])

    def pos(self, s):
        return self.L.fd_pos(self.h, s)

    def reset(self, s=-1):
        assert self.L.fd_reset(self.h, s) == 0

    def close(self):
        if self.h:
            self.L.fd_destroy(self.h)
            self.h = None


def decimate_plane(fs, fch, sch, x, cuts):
    """the emulation's decimate and carry stages alone over source frames x int16 [>= K(ticks - 1) * 1152][fch], the ticks cut into calls ->
    int16 [ticks][2304] (POISON where nothing is written)"""
    L = C.CDLL(str(build_emu()))
    L.fd_decimate_plane.argtypes = [C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    x = np.ascontiguousarray(x, dtype=np.int16)
    nt = sum(cuts)
    assert x.shape[0] >= K(nt - 1, *RATIOS[fs]) * N and x.shape[1] == fch
    out = np.full((nt, 2 * N), POISON, dtype=np.int16)
    cu = (C.c_int * len(cuts))(*cuts)
    rc = L.fd_decimate_plane(fs, ES, fch, sch, x.ctypes.data, len(cuts), cu, out.ctypes.data)
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
_shared = {}


def shared():
    """the stream set's inputs and oracle, once per process: fr / ln [NTICKS][ns][2][stride] and [NTICKS][ns][2], `used` the frames in wanted
    order, `want` the oracle's PCM [NTICKS][ns][2304] (zeros for the stream without a feed and where nothing is written)"""
    if not _shared:
        lists, used = slots_on_schedule(STREAMS)
        stride = max(F.slot_bytes(fcfg_of(st)) for st in STREAMS if st["feed"])
        fr, ln = slots_to_arrays(lists, stride)
        wantp = np.zeros((NTICKS, len(STREAMS), 2 * N), dtype=np.int16)
        for s, st in enumerate(STREAMS):
            if st["feed"]:
                wantp[:, s] = oracle_pcm(used[s], st)
        _shared.update(lists=lists, used=used, stride=stride, fr=fr, ln=ln, want=wantp)
    return _shared


def stream_configs(streams=STREAMS, psy=1):
    import odr_audioenc_amd as M
    return [M.StreamConfig(samplerate=ES, mode=st["mode"], bitrate=64, psy_model=psy) for st in streams]


def feed_config(st):
    import odr_audioenc_amd as M
    c = fcfg_of(st)
    return M.FeedConfig(samplerate=c["samplerate"], bitrate=c["bitrate"], channels=c["channels"])


def set_down_feeds(obj, streams=STREAMS):
    """the set's down feeds on a Batch"""
    for s, st in enumerate(streams):
        if st["feed"]:
            obj.set_down_feed(s, feed_config(st))
