"""Support for the frame check / decode tests (test_decode_emu.py, test_decode_gpu.py): the emulation of the decode kernels (compiled
into a temporary directory), an independent bit-level reader of Layer II frames in plain Python, and a numpy statement of
ISO/IEC 11172-3 2.4.3.3.4 + Annex 3-A.2 (requantisation and the synthesis filterbank, straight from the flow chart)."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"

REPORT_DTYPE = np.dtype([("status", np.uint32), ("crc_stored", np.uint16), ("crc_computed", np.uint16), ("mode", np.uint8),
                         ("mode_ext", np.uint8), ("audio_bits", np.uint16)])
FIELDS_DTYPE = np.dtype([("bit_alloc", np.uint8, (2, 32)), ("scfsi", np.uint8, (2, 32)), ("scalar", np.uint8, (2, 3, 32)),
                         ("subband", np.uint16, (2, 3, 12, 32))])
EMPTY, BAD_SYNC, HEADER_MISMATCH, BAD_CRC16, BAD_SCFCRC, SCFCRC_UNCHECKED, BAD_ALLOC, OVERRUN = (1 << i for i in range(8))
BAD_MASK = BAD_SYNC | HEADER_MISMATCH | BAD_CRC16 | BAD_SCFCRC | BAD_ALLOC | OVERRUN


def build_emu(outdir):
    """tests/emu/mp2_dec_emu.cpp + csrc/mp2_host.cpp -> outdir/libmp2decemu.so (the flags of tests/emu/Makefile)"""
    so = Path(outdir) / "libmp2decemu.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unused-function",
                    "-Wno-unused-variable", "-Wno-unknown-pragmas", "-shared", "-o", str(so), str(ROOT / "tests" / "emu" / "mp2_dec_emu.cpp"),
                    str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp"), "-lm"], check=True)
    return so


def build_san_driver(outdir):
    """tests/emu/mp2_dec_san_main.cpp + the emulation + csrc/mp2_host.cpp as ONE program under AddressSanitizer + UBSan (the flags of
    tools/emu_sanitize.sh; linked, not preloaded)"""
    exe = Path(outdir) / "mp2_dec_san"
    emu = ROOT / "tests" / "emu"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-mfma", "-ffp-contract=off",
                    "-fno-strict-aliasing", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas", "-o", str(exe),
                    str(emu / "mp2_dec_san_main.cpp"), str(emu / "mp2_dec_emu.cpp"), str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp"), "-lm"], check=True)
    return exe


def run_san_driver(exe, workdir, cfgs, cases):
    """cases: [(frames [nf][ns][stride] uint8, lens [nf][ns] int32 or None)] -> [(report, fields, pcm)] as the sanitized program wrote them"""
    import struct
    fin, fout = Path(workdir) / "cases.bin", Path(workdir) / "results.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ii", len(cfgs), len(cases)))
        for c in cfgs:
            f.write(struct.pack("<qiiii", c["samplerate"], ord(c["mode"]), c["kbps"], c.get("psy", 1), c.get("pad_len", 0)))
        for fr, ln in cases:
            f.write(struct.pack("<ii", fr.shape[0], 0 if ln is None else 1))
            f.write(np.ascontiguousarray(fr, dtype=np.uint8).tobytes())
            if ln is not None:
                f.write(np.ascontiguousarray(ln, dtype=np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")      # (nothing else of the environment changes)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    blob, pos, out = fout.read_bytes(), 0, []
    for fr, _ in cases:
        nf, ns = fr.shape[0], fr.shape[1]
        res = []
        for dt, shape in ((REPORT_DTYPE, (nf, ns)), (FIELDS_DTYPE, (nf, ns)), (np.dtype(np.int16), (nf, ns, 2, 1152))):
            n = dt.itemsize * int(np.prod(shape))
            res.append(np.frombuffer(blob[pos:pos + n], dtype=dt).reshape(shape))
            pos += n
        out.append(tuple(res))
    assert pos == len(blob)
    return out


class DecEmu:
    """N streams on the emulated decode path; decode() mirrors tlb_decode_host."""

    def __init__(self, so, cfgs):
        L = self.L = C.CDLL(str(so))
        L.dec_create.restype = C.c_void_p
        L.dec_create.argtypes = [C.c_int] + [C.c_void_p] * 6
        L.dec_destroy.argtypes = [C.c_void_p]
        for f in ("dec_out_stride", "dec_bad_frames"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.dec_bad_frames.restype = C.c_long
        for f in ("dec_frame_bytes", "dec_pads", "dec_reset"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_int]
        L.dec_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.dec_sizeof_report() == REPORT_DTYPE.itemsize and L.dec_sizeof_fields() == FIELDS_DTYPE.itemsize
        n = self.n = len(cfgs)
        fs = (C.c_long * n)(*[c["samplerate"] for c in cfgs])
        mode = bytes(ord(c["mode"]) for c in cfgs)
        kb = (C.c_int * n)(*[c["kbps"] for c in cfgs])
        psy = (C.c_int * n)(*[c.get("psy", 1) for c in cfgs])
        pad = (C.c_int * n)(*[c.get("pad_len", 0) for c in cfgs])
        err = C.c_int(0)
        self.h = L.dec_create(n, fs, mode, kb, psy, pad, C.byref(err))
        assert self.h, err.value
        self.stride = L.dec_out_stride(self.h)
        self.frame_bytes = [L.dec_frame_bytes(self.h, s) for s in range(n)]

    def decode(self, frames, lens, want_fields=True, want_pcm=False):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        assert frames.shape == (nf, self.n, self.stride)
        ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
        rep = np.zeros((nf, self.n), dtype=REPORT_DTYPE)
        fl = np.zeros((nf, self.n), dtype=FIELDS_DTYPE) if want_fields else None
        pcm = np.zeros((nf, self.n, 2, 1152), dtype=np.int16) if want_pcm else None
        rc = self.L.dec_decode(self.h, frames.ctypes.data, None if ln is None else ln.ctypes.data, nf, rep.ctypes.data,
                               None if fl is None else fl.ctypes.data, None if pcm is None else pcm.ctypes.data)
        assert rc == 0, rc
        return rep, fl, pcm

    def reset(self, s=-1):
        assert self.L.dec_reset(self.h, s) == 0

    def bad_frames(self):
        return int(self.L.dec_bad_frames(self.h))

    def close(self):
        if self.h:
            self.L.dec_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------------------------------------------------------------------------
# goldens
def golden_names():
    return sorted(p.stem for p in GOLDEN.glob("p*.npz"))


def golden_cfg(g):
    fs, mode, kbps, psy, kind, seed, pad_len, nframes = (int(x) for x in g["cfg"])
    return dict(samplerate=fs, mode=chr(mode), kbps=kbps, psy=psy, pad_len=pad_len, kind=kind, seed=seed, nframes=nframes)


def frame_bytes_of(cfg):
    """bytes of a frame without its padding slot: 1152 samples at `kbps`, i.e. 144 * bitrate / fs, at the half rates too (2.4.3.1)"""
    return 144000 * cfg["kbps"] // cfg["samplerate"]


def cut_frames(data, cfg):
    """the reference's byte stream -> its frames, by the frame length and each header's padding bit"""
    data = bytes(data)
    base, out, pos = frame_bytes_of(cfg), [], 0
    while pos < len(data):
        n = base + ((data[pos + 2] >> 1) & 1)
        out.append(data[pos:pos + n])
        pos += n
    assert pos == len(data)
    return out


def batch_arrays(frame_lists, stride):
    """per stream a list of frames -> frames [nf][ns][stride], lens [nf][ns] (streams with fewer frames: empty slots at the end)"""
    nf, ns = max(len(f) for f in frame_lists), len(frame_lists)
    frames = np.zeros((nf, ns, stride), dtype=np.uint8)
    lens = np.zeros((nf, ns), dtype=np.int32)
    for s, fl in enumerate(frame_lists):
        for f, b in enumerate(fl):
            frames[f, s, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            lens[f, s] = len(b)
    return frames, lens


# ---------------------------------------------------------------------------------------------------------------------------------
# The independent reader: ISO/IEC 11172-3 2.4.1 / 2.4.2 and 13818-3 2.4 over np.unpackbits.  Allocation tables B.2a-d and the LSF table
# as the REFERENCE holds them in memory (tests/golden/tables_rates.npz: nbal per line, line per (table, subband), sblimit per table).
_T = None


def _tables():
    global _T
    if _T is None:
        z = np.load(GOLDEN / "tables_rates.npz")
        _T = dict(nbal=z["alloc_nbal"].astype(int), sblimit=z["alloc_table_sblimit"].astype(int), line=z["alloc_line"].astype(int).reshape(5, 32),
                  step_index=z["alloc_step_index"].astype(int).reshape(9, 16), bits=z["alloc_bits"].astype(int), group=z["alloc_group"].astype(int),
                  steps=z["alloc_steps"].astype(int))
    return _T


def pick_table(cfg):
    """2.4.2.3 (which of B.2a-d) / 13818-3 (B.1 for the half rates)"""
    fs, nch = cfg["samplerate"], 1 if cfg["mode"] == "m" else 2
    if fs < 32000:
        return 4
    per_ch = cfg["kbps"] // nch
    if (fs == 48000 and per_ch >= 56) or 56 <= per_ch <= 80:
        return 0
    if fs != 48000 and per_ch >= 96:
        return 1
    if fs != 32000 and per_ch <= 48:
        return 2
    return 3


def dab_ext_of(cfg):
    """ScF-CRC bytes of a frame: 4, or 2 for MPEG-1 below 56 kbps per channel (ETSI EN 300 401 B.3)"""
    nch = 1 if cfg["mode"] == "m" else 2
    return 2 if cfg["samplerate"] >= 32000 and cfg["kbps"] // nch < 56 else 4


def _crc(bits, poly, width, init):
    crc, top, mask = init, 1 << (width - 1), (1 << width) - 1
    for b in bits:
        carry = 1 if crc & top else 0
        crc = (crc << 1) & mask
        if carry ^ int(b):
            crc ^= poly
    return crc


def read_frame(frame, cfg):
    """-> dict(mode, mode_ext, jsbound, bit_alloc [2][32], scfsi, scalar [2][3][32], subband [2][3][12][32], crc_stored, crc_computed,
    scfcrc [dab_ext] in group order, audio_bits).  Cells the frame does not transmit are 0."""
    T = _tables()
    bits = np.unpackbits(np.frombuffer(bytes(frame), dtype=np.uint8))

    def get(pos, n):
        v = 0
        for b in bits[pos:pos + n]:
            v = (v << 1) | int(b)
        return v
    tab = pick_table(cfg)
    sblimit, nch = int(T["sblimit"][tab]), 1 if cfg["mode"] == "m" else 2
    mode, mode_ext = get(24, 2), get(26, 2)
    jsbound = min(4 * (mode_ext + 1), sblimit) if mode == 1 else sblimit
    ba = np.zeros((2, 32), dtype=int); scfsi = np.zeros((2, 32), dtype=int); scalar = np.zeros((2, 3, 32), dtype=int)
    sub = np.zeros((2, 3, 12, 32), dtype=int)
    pos = 48
    for sb in range(sblimit):
        nb = int(T["nbal"][T["line"][tab][sb]])
        for ch in range(nch if sb < jsbound else 1):
            ba[ch][sb] = get(pos, nb); pos += nb
        if sb >= jsbound and nch == 2:
            ba[1][sb] = ba[0][sb]
    for sb in range(sblimit):
        for ch in range(nch):
            if ba[ch][sb]:
                scfsi[ch][sb] = get(pos, 2); pos += 2
    crc_computed = _crc(np.concatenate([bits[16:32], bits[48:pos]]), 0x8005, 16, 0xffff)
    for sb in range(sblimit):
        for ch in range(nch):
            if ba[ch][sb]:
                k = int(scfsi[ch][sb])
                n = (3, 2, 1, 2)[k]
                v = [get(pos + 6 * i, 6) for i in range(n)]; pos += 6 * n
                scalar[ch, :, sb] = {0: v, 1: [v[0], v[0], v[-1]], 2: [v[0]] * 3, 3: [v[0], v[-1], v[-1]]}[k]
    for gr in range(3):
        for tr in range(4):
            for sb in range(sblimit):
                for ch in range(nch if sb < jsbound else 1):
                    if ba[ch][sb]:
                        q = int(T["step_index"][T["line"][tab][sb]][ba[ch][sb]])
                        nb, steps = int(T["bits"][q]), int(T["steps"][q])
                        if int(T["group"][q]) == 3:
                            v = [get(pos + nb * i, nb) for i in range(3)]; pos += 3 * nb
                        else:
                            c = get(pos, nb); pos += nb
                            v = [c % steps, (c // steps) % steps, c // (steps * steps)]
                        sub[ch, gr, 3 * tr:3 * tr + 3, sb] = v
    # ScF-CRC (ETSI EN 300 401 B.3): CRC-8 (x^8 + x^4 + x^3 + x^2 + 1, zero preset) over the three MSBs of the transmitted scalefactors
    # of subbands 0..3, 4..7, 8..15, 16..29
    n_ext, scfcrc = dab_ext_of(cfg), []
    bounds = [0, 4, 8, 16, 30]
    for g in range(n_ext):
        rec = []
        for sb in range(bounds[g], min(bounds[g + 1], sblimit)):
            for ch in range(nch):
                if ba[ch][sb]:
                    idx = {0: [0, 1, 2], 1: [0, 2], 2: [0], 3: [0, 2]}[int(scfsi[ch][sb])]
                    for i in idx:
                        m = int(scalar[ch][i][sb]) >> 3
                        rec += [(m >> 2) & 1, (m >> 1) & 1, m & 1]
        scfcrc.append(_crc(rec, 0x1d, 8, 0))
    return dict(mode=mode, mode_ext=mode_ext, jsbound=jsbound, nch=nch, sblimit=sblimit, tab=tab, bit_alloc=ba, scfsi=scfsi, scalar=scalar,
                subband=sub, crc_stored=get(32, 16), crc_computed=crc_computed, scfcrc=scfcrc, audio_bits=pos)


def stored_scfcrc(frame, cfg):
    """the ScF-CRC bytes in a frame's tail, in group order (they protect the NEXT frame; the last frame of a stream carries its own)"""
    n = dab_ext_of(cfg)
    tail = bytes(frame)[len(frame) - 2 - n:len(frame) - 2]
    return [tail[n - 1 - g] for g in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------
# ISO/IEC 11172-3 2.4.3.3.4 and Annex 3-A.2 in numpy.  Table 3-B.4 (C and D per number of steps) as printed in the standard.
RQ = {3: (1.33333333333, 0.50000000000), 5: (1.60000000000, 0.50000000000), 7: (1.14285714286, 0.25000000000),
      9: (1.77777777777, 0.50000000000), 15: (1.06666666666, 0.12500000000), 31: (1.03225806452, 0.06250000000),
      63: (1.01587301587, 0.03125000000), 127: (1.00787401575, 0.01562500000), 255: (1.00392156863, 0.00781250000),
      511: (1.00195694716, 0.00390625000), 1023: (1.00097751711, 0.00195312500), 2047: (1.00048851979, 0.00097656250),
      4095: (1.00024420024, 0.00048828125), 8191: (1.00012208522, 0.00024414063), 16383: (1.00006103888, 0.00012207031),
      32767: (1.00003051851, 0.00006103516), 65535: (1.00001525902, 0.00003051758)}


def requantise(fields, info):
    """fields of one frame (bit_alloc, scalar, subband as read) -> s'[ch][36][32] (fraction * scalefactor).  `info`: what read_frame
    says of the frame's shape (tab, nch, sblimit, jsbound)."""
    T = _tables()
    multiple = np.load(GOLDEN / "tables_48k.npz")["multiple"]
    out = np.zeros((2, 36, 32))
    for ch in range(info["nch"]):
        for sb in range(info["sblimit"]):
            ba = int(fields["bit_alloc"][ch][sb])
            if not ba:
                continue
            steps = int(T["steps"][T["step_index"][T["line"][info["tab"]][sb]][ba]])
            nb = steps.bit_length()                                  # bits of one sample code
            cc, dd = RQ[steps]
            src = 0 if sb >= info["jsbound"] else ch                 # joint stereo: the samples travel once, under channel 0
            for gr in range(3):
                code = fields["subband"][src][gr][:, sb].astype(np.int64)
                inv = code ^ (1 << (nb - 1))                         # invert the MSB ...
                frac = np.where(inv >= (1 << (nb - 1)), inv - (1 << nb), inv) / float(1 << (nb - 1))      # ... two's complement fraction
                out[ch, 12 * gr:12 * gr + 12, sb] = cc * (frac + dd) * multiple[int(fields["scalar"][ch][gr][sb])]
    return out


class Synth:
    """figure 3-A.2, one channel: V shifted by 64, matrixed, U built, windowed, 32 samples out"""
    i, k = np.meshgrid(np.arange(64), np.arange(32), indexing="ij")
    N = np.cos((16 + i) * (2 * k + 1) * np.pi / 64.0)
    D = 32.0 * np.load(GOLDEN / "tables_48k.npz")["enwindow"]

    def __init__(self):
        self.V = np.zeros(1024)

    def step(self, s):
        self.V[64:] = self.V[:-64].copy()
        self.V[:64] = self.N @ s
        U = np.zeros(512)
        for i in range(8):
            U[64 * i:64 * i + 32] = self.V[128 * i:128 * i + 32]
            U[64 * i + 32:64 * i + 64] = self.V[128 * i + 96:128 * i + 128]
        return (U * self.D).reshape(16, 32).sum(axis=0)

    def frame(self, s36):
        return np.concatenate([self.step(s) for s in s36])


def to_int16(x):
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
