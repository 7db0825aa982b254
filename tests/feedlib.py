"""Support for the Layer II feed tests (test_feed_abi.py, test_feed_emu.py, test_feed_gpu.py, and through feedadaptlib test_feed_adapt_*.py):
the emulation of the feed kernels, strict and adapted (compiled into a temporary directory), its sanitizer driver and ctypes layer, the numpy statement of a feed's decode built on declib's reader, requantiser and synthesis, the three
transforms that make a project-encoded frame "foreign" without changing its audio, and the cases and hostile inputs the tests share.
A plain module: nothing here is collected by pytest."""
import ctypes as C
import os
import struct
import subprocess
from pathlib import Path

import numpy as np

import declib as D

ROOT = D.ROOT
REPORT_DTYPE = D.REPORT_DTYPE
POISON = 0x1111                                                  # what output buffers hold before a feed call: slots the kernel must not touch keep it

# (samplerate, mode of the SOURCE encoder, kbps, pcmgen kind): the feed's configuration is (samplerate, kbps, channels of the mode).
# 48 kHz 'j' 128 with pcmgen kind 3 switches between joint stereo and stereo from frame to frame; 44.1 kHz has padding slots; 32 kHz 384 is
# the longest frame there is.
CASES = [(48000, "s", 192, 0), (48000, "j", 128, 3), (48000, "d", 64, 2), (48000, "m", 64, 4), (44100, "s", 128, 5), (32000, "s", 384, 7),
         (24000, "m", 32, 0), (16000, "s", 64, 2)]
NFRAMES = 6
VARIANTS = ("plain", "strip_crc", "set_free_bits", "scribble_tail")


def feed_cfg_of(case):
    fs, mode, kbps, _ = case
    return dict(samplerate=fs, bitrate=kbps, channels=1 if mode == "m" else 2)


def reader_cfg(fcfg):
    """the feed's configuration as declib's reader takes one: the mode only says how many channels there are"""
    return dict(samplerate=fcfg["samplerate"], kbps=fcfg["bitrate"], mode="m" if fcfg["channels"] == 1 else "s")


def slot_bytes(fcfg):
    """the feed's longest frame, with its padding slot where the rate has one, rounded up to 4"""
    n = D.frame_bytes_of(reader_cfg(fcfg)) + (1 if fcfg["samplerate"] in (44100, 22050) else 0)
    return (n + 3) & ~3


def case_pcm(i, case, nframes=NFRAMES):
    from pcmgen import gen_pcm
    return gen_pcm(4100 + i, case[3], 0, nframes)


def oracle_frames(case, pcm):
    """the oracle encoder's frames for [nframes][2][1152] of PCM (CPU)"""
    import oraclelib as O
    fs, mode, kbps, _ = case
    data, _ = O.oracle_stream(pcm, samplerate=fs, mode=mode, kbps=kbps, psy=1)
    fr = D.cut_frames(data, dict(samplerate=fs, kbps=kbps))
    assert len(fr) == pcm.shape[0]
    return fr


# ---------------------------------------------------------------------------------------------------------------------------------
# the transforms: a project-encoded frame made foreign, its audio unchanged
def _bits(frame):
    return np.unpackbits(np.frombuffer(bytes(frame), dtype=np.uint8))


def _has_crc(frame):
    return not (bytes(frame)[1] & 1)


def _with_crc_gap(frame):
    """a frame without protection as declib.read_frame can read it: 16 bits put back behind the header"""
    if _has_crc(frame):
        return bytes(frame)
    b = _bits(frame)
    return np.packbits(np.concatenate([b[:32], np.zeros(16, dtype=np.uint8), b[32:]])).tobytes()


def read_feed_frame(frame, fcfg):
    """declib.read_frame under the feed's configuration; audio_bits counts the frame's own bits (no CRC-16: 16 fewer)"""
    info = D.read_frame(_with_crc_gap(frame), reader_cfg(fcfg))
    if not _has_crc(frame):
        info["audio_bits"] -= 16
    return info


def strip_crc(frame):
    """set the protection bit, drop the 16 CRC bits, shift the rest up, zero-fill the tail"""
    b = _bits(frame)
    assert b[15] == 0
    b = np.concatenate([b[:32], b[48:], np.zeros(16, dtype=np.uint8)])
    b[15] = 1
    return np.packbits(b).tobytes()


def set_free_bits(frame, fcfg):
    """set private / copyright / original / emphasis, and recompute the CRC-16 (declib's _crc, through read_frame)"""
    b = _bits(frame)
    b[23] = 1; b[28] = 1; b[29] = 1; b[31] = 1
    crc = D.read_frame(np.packbits(b).tobytes(), reader_cfg(fcfg))["crc_computed"]
    b[32:48] = [(crc >> (15 - i)) & 1 for i in range(16)]
    return np.packbits(b).tobytes()


def scribble_tail(frame, fcfg, rng):
    """random bytes over the whole bytes behind audio_bits"""
    first = (read_feed_frame(frame, fcfg)["audio_bits"] + 7) // 8
    out = bytearray(frame)
    assert first < len(out)
    out[first:] = rng.integers(0, 256, len(out) - first, dtype=np.uint8).tobytes()
    return bytes(out)


def variants_of(frames, fcfg, seed=9):
    """-> {variant: frames}: untouched and under each transform"""
    rng = np.random.default_rng(seed)
    return dict(plain=list(frames), strip_crc=[strip_crc(f) for f in frames], set_free_bits=[set_free_bits(f, fcfg) for f in frames],
                scribble_tail=[scribble_tail(f, fcfg, rng) for f in frames])


# ---------------------------------------------------------------------------------------------------------------------------------
# the numpy statement: ISO/IEC 11172-3 2.4.3.3.4 + Annex 3-A.2 (declib) over a feed's frames, interleaved as the ingest reads them
def numpy_feed_pcm(frames, fcfg):
    """frames: bytes per slot, or None for a slot that decodes to silence (empty, or a frame that does not pass) -> int16 [nframes][2304]"""
    nch = fcfg["channels"]
    syn = [D.Synth() for _ in range(nch)]
    out = np.zeros((len(frames), 2304), dtype=np.int16)
    for f, fr in enumerate(frames):
        if fr is None:
            for ch in range(nch):
                syn[ch].frame(np.zeros((36, 32)))                # silence in the successor's filter history
            continue
        info = read_feed_frame(fr, fcfg)
        s = D.requantise(info, info)
        for ch in range(nch):
            out[f, ch:1152 * nch:nch] = D.to_int16(syn[ch].frame(s[ch]))
    return out


def interleave(planar, nch):
    """[.., 2, 1152] as tlb_decode_* writes it -> [.., 2304] as a feed writes it (a one-channel stream: 1152 samples, then zeros)"""
    planar = np.asarray(planar)
    out = np.zeros(planar.shape[:-2] + (2304,), dtype=np.int16)
    if nch == 2:
        out[..., 0::2] = planar[..., 0, :]
        out[..., 1::2] = planar[..., 1, :]
    else:
        out[..., :1152] = planar[..., 0, :]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# hostile input: [(name, fn(list of frames) -> list of (bytes, length)), flags that must be set] over a stream's six good frames; the damaged
# slot is HOSTILE_SLOT, its successor must come out as after silence
HOSTILE_SLOT = 3


def hostile_inputs(frames, fcfg, stride):
    """-> [(name, slots [(bytes, len)], must)]: one damaged slot per input"""
    rng = np.random.default_rng(31)
    good = [(f, len(f)) for f in frames]
    fr = frames[HOSTILE_SLOT]
    info = read_feed_frame(fr, fcfg)
    T = D._tables()
    out = []

    def put(name, b, n, must):
        slots = list(good)
        slots[HOSTILE_SLOT] = (bytes(b), n)
        out.append((name, slots, must))
    put("random", rng.integers(0, 256, len(fr), dtype=np.uint8).tobytes(), len(fr), D.BAD_MASK)
    for n in range(32, len(fr), 32):
        put(f"trunc{n}", fr[:n], n, D.OVERRUN)
    b = bytearray(fr); b[2] ^= 0x10                              # a bitrate-index bit
    put("bitrate", b, len(fr), D.HEADER_MISMATCH)
    b = bytearray(fr); b[2] ^= 0x04                              # a sampling-frequency-index bit
    put("rate", b, len(fr), D.HEADER_MISMATCH)
    b = bytearray(fr); b[3] = (b[3] & 0x3f) | ((0 if fcfg["channels"] == 1 else 3) << 6)      # mono on a two-channel feed, stereo on a one-channel one
    put("mode", b, len(fr), D.HEADER_MISMATCH)
    bits = _bits(fr)                                             # a bit_alloc field forced to all ones: the first one (subband 0, channel 0)
    nb = int(T["nbal"][T["line"][info["tab"]][0]])
    bits[48:48 + nb] = 1
    put("alloc", np.packbits(bits).tobytes(), len(fr), D.BAD_CRC16)
    return out


def slots_to_arrays(slot_lists, stride):
    """per stream a list of (bytes, len) -> frames [nf][ns][stride], lens [nf][ns]"""
    nf, ns = len(slot_lists[0]), len(slot_lists)
    frames = np.zeros((nf, ns, stride), dtype=np.uint8)
    lens = np.zeros((nf, ns), dtype=np.int32)
    for s, sl in enumerate(slot_lists):
        for f, (b, n) in enumerate(sl):
            frames[f, s, :len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
            lens[f, s] = n
    return frames, lens


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation: ONE for strict and adapted feeds (tests/emu/mp2_feed_emu.cpp); feedadaptlib adds what is specific to adapted feeds.
# A stream is a row (fcfg or None, adapted, the stream's rate, the stream's channels); a strict feed's stream has the feed's rate and channels.
_FLAGS = ["-std=c++17", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas",
          "-Wno-unused-but-set-variable", "-Wno-maybe-uninitialized"]
_SRC = [str(ROOT / "tests" / "emu" / "mp2_feed_emu.cpp"), str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp")]


def strict_rows(fcfgs):
    return [(c, 0, c["samplerate"] if c else 0, c["channels"] if c else 0) for c in fcfgs]


def build_emu(outdir):
    """tests/emu/mp2_feed_emu.cpp + csrc/mp2_host.cpp -> outdir/libmp2feedemu.so"""
    so = Path(outdir) / "libmp2feedemu.so"
    subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + _FLAGS + ["-o", str(so)] + _SRC + ["-lm"], check=True)
    return so


def build_san_driver(outdir):
    """tests/emu/mp2_feed_san_main.cpp + the emulation + csrc/mp2_host.cpp as ONE program under AddressSanitizer + UBSan (linked, not preloaded)"""
    exe = Path(outdir) / "mp2_feed_san"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + _FLAGS + ["-o", str(exe),
                    str(ROOT / "tests" / "emu" / "mp2_feed_san_main.cpp")] + _SRC + ["-lm"], check=True)
    return exe


def run_san_rows(exe, workdir, rows, cases):
    """cases: [[(frames, lens), ...]]: per case the calls of one run from the reset -> per case [(report, pcm)] per call, as the sanitized
    program wrote them (every sample POISON before each call)"""
    fin, fout = Path(workdir) / "cases.bin", Path(workdir) / "results.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ii", len(rows), len(cases)))
        for c, adapt, rate, nch in rows:
            f.write(struct.pack("<qiiiqi", c["samplerate"] if c else 0, c["bitrate"] if c else 0, c["channels"] if c else 0, int(adapt), rate, nch))
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
        res = []
        for fr, _ in calls:
            nf, ns = fr.shape[0], fr.shape[1]
            one = []
            for dt, shape in ((REPORT_DTYPE, (nf, ns)), (np.dtype(np.int16), (nf, ns, 2304))):
                n = dt.itemsize * int(np.prod(shape))
                one.append(np.frombuffer(blob[pos:pos + n], dtype=dt).reshape(shape))
                pos += n
            res.append(tuple(one))
        out.append(res)
    assert pos == len(blob)
    return out


def run_san_driver(exe, workdir, fcfgs, cases):
    """fcfgs: per stream a feed configuration or None; cases: [(frames, lens)] -> [(report, pcm)] as the sanitized program wrote them"""
    return [calls[0] for calls in run_san_rows(exe, workdir, strict_rows(fcfgs), [[c] for c in cases])]


class FeedEmu:
    """N streams on the emulated feed path.  Either fcfgs: per stream dict(samplerate, bitrate, channels) or None (no feed), every feed a
    strict one; or rows (fcfgs is then not read): per stream the tuple (fcfg or None, set through the adapted entry point, the stream's
    rate, the stream's channels), as feedadaptlib.rows_of makes them.  decode() mirrors tlb_feed_host with an output buffer that holds
    POISON before the call."""

    def __init__(self, so, fcfgs, rows=None):
        L = self.L = C.CDLL(str(so))
        L.feed_create.restype = C.c_void_p
        L.feed_create.argtypes = [C.c_int] + [C.c_void_p] * 7
        L.feed_destroy.argtypes = [C.c_void_p]
        L.feed_stride.argtypes = [C.c_void_p]
        L.feed_reset.argtypes = [C.c_void_p, C.c_int]
        L.feed_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert L.feed_sizeof_report() == REPORT_DTYPE.itemsize
        rows = strict_rows(fcfgs) if rows is None else rows
        n = self.n = len(rows)
        fs = (C.c_long * n)(*[c["samplerate"] if c else 0 for c, _, _, _ in rows])
        kb = (C.c_int * n)(*[c["bitrate"] if c else 0 for c, _, _, _ in rows])
        ch = (C.c_int * n)(*[c["channels"] if c else 0 for c, _, _, _ in rows])
        ad = (C.c_int * n)(*[int(a) for _, a, _, _ in rows])
        er = (C.c_long * n)(*[r for _, _, r, _ in rows])
        en = (C.c_int * n)(*[k for _, _, _, k in rows])
        err = C.c_int(0)
        self.h = L.feed_create(n, fs, kb, ch, ad, er, en, C.byref(err))
        assert self.h, err.value
        self.stride = L.feed_stride(self.h)

    def decode(self, frames, lens, init=None):
        """init: what the output buffer holds before the call (None: POISON everywhere)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        assert frames.shape == (nf, self.n, self.stride)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        assert ln.shape == (nf, self.n)
        rep = np.zeros((nf, self.n), dtype=REPORT_DTYPE)
        pcm = np.full((nf, self.n, 2304), POISON, dtype=np.int16) if init is None else np.array(init, dtype=np.int16, order="C", copy=True)
        assert pcm.shape == (nf, self.n, 2304)
        rc = self.L.feed_decode(self.h, frames.ctypes.data, ln.ctypes.data, nf, pcm.ctypes.data, rep.ctypes.data)
        assert rc == 0, rc
        return pcm, rep

    def reset(self, s=-1):
        assert self.L.feed_reset(self.h, s) == 0

    def close(self):
        if self.h:
            self.L.feed_destroy(self.h)
            self.h = None


def expected_written(pcm, fcfgs):
    """the part of an output buffer a feed call writes: per stream the first 1152 * channels samples of a fed stream's slots"""
    m = np.zeros(pcm.shape, dtype=bool)
    for s, c in enumerate(fcfgs):
        if c:
            m[:, s, :1152 * c["channels"]] = True
    return m
