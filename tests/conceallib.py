"""Support for the feed concealment tests (test_conceal_emu.py, test_conceal_abi.py, test_conceal_gpu.py, test_example_conceal.py): the
ORACLE -- a sequential per-stream loop over the definition in csrc/mp2_conceal.h, built on feedlib.read_feed_frame and declib's requantise,
Synth and to_int16 --, the loss scenarios the tests share, and, following feedlib, the emulation of the kernels (compiled into a temporary
directory), its ctypes layer and its sanitizer driver.  A plain module: nothing here is collected by pytest."""
import ctypes as C
import os
import struct
import subprocess
from pathlib import Path

import numpy as np

import declib as D
import feedlib as F

ROOT = D.ROOT
POISON = F.POISON
MUTE = 0xFFFFFFFF
RECORD_FIELDS = ("frames", "passed", "concealed", "muted", "runs", "longest", "run", "offset")
RECORD_DTYPE = np.dtype([(n, np.uint32) for n in RECORD_FIELDS])
NSLOTS = 12
CASES = F.CASES[:6]            # mono, joint, dual, 44.1 kHz with a padding slot, 32 kHz at 384 kbps
LOST_BITS = D.BAD_MASK | D.EMPTY


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition
def offset(k, hold, step):
    return 0 if k == 0 else step * k if k <= hold else MUTE


def at_offset(info, o):
    """G at offset o: a copy of the parsed frame with every scalefactor index raised, none beyond 63"""
    out = dict(info)
    out["scalar"] = np.full_like(info["scalar"], 63) if o == MUTE else np.minimum(info["scalar"] + o, 63)
    return out


def _synth(info, hist, nch):
    """one frame over a history that is a parsed frame or None (silence) -> int16 [2304], interleaved as the ingest reads it"""
    out = np.zeros(2304, dtype=np.int16)
    s = D.requantise(info, info)
    h = D.requantise(hist, hist) if hist is not None else None
    for ch in range(nch):
        syn = D.Synth()
        if h is not None:
            syn.frame(h[ch])
        out[ch:1152 * nch:nch] = D.to_int16(syn.frame(s[ch]))
    return out


def oracle_stream(slots, lost, fcfg, hold, step):
    """slots: per slot (bytes, len); lost: per slot whether it is lost -> (pcm int16 [n][2304], record).  What lies behind a one-channel
    feed's 1152 samples is 0 here and not the kernels' to write."""
    nch = fcfg["channels"]
    out = np.zeros((len(slots), 2304), dtype=np.int16)
    rec = dict.fromkeys(RECORD_FIELDS, 0)
    G, k, before = None, 0, None                                 # before: the slot before when it passed
    for f, ((b, n), gone) in enumerate(zip(slots, lost)):
        rec["frames"] += 1
        if gone:
            k += 1
            rec["runs"] += k == 1
            rec["longest"] = max(rec["longest"], k)
            if G is not None and offset(k - 1, hold, step) != MUTE:
                out[f] = _synth(at_offset(G, offset(k, hold, step)), at_offset(G, offset(k - 1, hold, step)), nch)
                rec["concealed"] += 1
            else:
                rec["muted"] += 1
            before = None
            continue
        info = F.read_feed_frame(bytes(b)[:n], fcfg)
        if k > 0:
            hist = at_offset(G, offset(k, hold, step)) if G is not None and offset(k, hold, step) != MUTE else None
        else:
            hist = before
        out[f] = _synth(info, hist, nch)
        G, k, before = info, 0, info
        rec["passed"] += 1
    rec["run"], rec["offset"] = k, offset(k, hold, step)
    return out, np.array(tuple(rec[n] for n in RECORD_FIELDS), dtype=RECORD_DTYPE)


def oracle_record(lost, hold, step):
    """the record alone, for a sequence of lost flags and a first slot that has a G whenever a slot before it passed"""
    rec = dict.fromkeys(RECORD_FIELDS, 0)
    have, k = False, 0
    for gone in lost:
        rec["frames"] += 1
        if not gone:
            have, k = True, 0
            rec["passed"] += 1
            continue
        k += 1
        rec["runs"] += k == 1
        rec["longest"] = max(rec["longest"], k)
        rec["concealed" if have and k - 1 <= hold else "muted"] += 1
    rec["run"], rec["offset"] = k, offset(k, hold, step)
    return np.array(tuple(rec[n] for n in RECORD_FIELDS), dtype=RECORD_DTYPE)


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenarios: one stream each, NSLOTS slots each.  A scenario is (name, hold, step, ways): per slot None (the good frame) or the way
# it is lost.
def _flip_crc(fr):
    b = bytearray(fr); b[5] ^= 0x01
    return bytes(b), len(fr)


def _break_sync(fr):
    b = bytearray(fr); b[0] = 0x7f
    return bytes(b), len(fr)


WAYS = {
    "empty": lambda fr: (b"", 0),
    "crc": _flip_crc,
    "sync": _break_sync,
    "trunc": lambda fr: (fr[:len(fr) // 2], len(fr) // 2),
    "long": lambda fr: (fr + b"\0\0\0\0", len(fr) + 4),          # (a slot longer than the frame; the batch's stride must have the room)
}
HOSTILE = ("random", "bitrate", "alloc")                         # of feedlib.hostile_inputs: the damaged slot's bytes


def _run(first, n, way="empty"):
    return [way if first <= f < first + n else None for f in range(NSLOTS)]


def scenarios(hold=4, step=3, long_ok=True):
    lng = "long" if long_ok else "sync"
    out = [("none", hold, step, [None] * NSLOTS),
           ("one", hold, step, _run(5, 1)),
           ("hold", hold, step, _run(2, hold)),
           ("hold+1", hold, step, _run(2, hold + 1)),
           ("hold+3", hold, step, _run(2, hold + 3)),
           ("first", hold, step, _run(0, 2)),
           ("alternating", hold, step, ["crc" if f % 2 else None for f in range(NSLOTS)]),
           ("two_runs", hold, step, [w or v for w, v in zip(_run(1, 3), _run(5, 3, "sync"))]),
           ("ways", hold, step, [None, "empty", None, "crc", "sync", None, "trunc", lng, None, "random", "bitrate", "alloc"])]
    for h in (1, 4, 16):
        for st in (1, 3, 21):
            if (h, st) != (hold, step):
                out.append((f"h{h}s{st}", h, st, _run(2, min(h + 3, 8), "crc")))
    return out


_FRAMES = {}


def case_frames(i):
    """the oracle encoder's NSLOTS frames of case i (CPU), once"""
    if i not in _FRAMES:
        case = CASES[i]
        _FRAMES[i] = F.oracle_frames(case, F.case_pcm(i, case, NSLOTS))
    return _FRAMES[i]


def slots_of(frames, ways, fcfg):
    """-> per slot (bytes, len)"""
    hostile = None
    out = []
    for f, (fr, way) in enumerate(zip(frames, ways)):
        if way is None:
            out.append((fr, len(fr)))
        elif way in WAYS:
            out.append(WAYS[way](fr))
        else:
            if hostile is None:                                  # the damage feedlib does to ITS slot, done to this one
                hostile = {}
            if f not in hostile:
                six = [fr] * F.NFRAMES
                hostile[f] = {n: sl[F.HOSTILE_SLOT] for n, sl, _ in F.hostile_inputs(six, fcfg, F.slot_bytes(fcfg))}
            out.append(hostile[f][way])
    return out


def scenario_batch(case_ids):
    """every scenario of the named cases as one stream each, then per case a fed stream WITHOUT concealment (the "ways" losses) and at the
    very end an all-empty wide feed and a stream without a feed -> list of dict(case, name, fcfg, hold, step, slots, lost)"""
    rows = []
    for i in case_ids:
        fcfg = F.feed_cfg_of(CASES[i])
        frames = case_frames(i)
        sc = scenarios(long_ok=F.slot_bytes(fcfg) < 1728)
        for name, hold, step, ways in sc:
            rows.append(dict(case=i, name=name, fcfg=fcfg, hold=hold, step=step, slots=slots_of(frames, ways, fcfg), lost=[w is not None for w in ways]))
        ways = sc[8][3]
        rows.append(dict(case=i, name="unconcealed", fcfg=fcfg, hold=0, step=0, slots=slots_of(frames, ways, fcfg), lost=[w is not None for w in ways]))
    # a fed stream of the longest frame there is, every slot empty: the batch's slots are then wide enough for a slot longer than its frame
    rows.append(dict(case=None, name="wide", fcfg=F.feed_cfg_of(CASES[5]), hold=0, step=0, slots=[(b"", 0)] * NSLOTS, lost=[True] * NSLOTS))
    rows.append(dict(case=None, name="unfed", fcfg=None, hold=0, step=0, slots=[(b"", 0)] * NSLOTS, lost=[True] * NSLOTS))
    return rows


_ORACLE = {}


def oracle_of(row):
    """(pcm, record) of a scenario row, computed once and shared (do not write to it).  An unconcealed row: feedlib's numpy statement, and
    an all-zero record"""
    key = (row["case"], row["name"])
    if key not in _ORACLE:
        if row["hold"]:
            _ORACLE[key] = oracle_stream(row["slots"], row["lost"], row["fcfg"], row["hold"], row["step"])
        else:
            pcm = F.numpy_feed_pcm([None if gone else bytes(b)[:n] for (b, n), gone in zip(row["slots"], row["lost"])], row["fcfg"])
            _ORACLE[key] = (pcm, np.zeros((), dtype=RECORD_DTYPE))
        _ORACLE[key][0].setflags(write=False)
    return _ORACLE[key]


def batch_arrays(rows, stride):
    return F.slots_to_arrays([r["slots"] for r in rows], stride)


CUTS = {"1": [1] * 12, "2": [2] * 6, "3": [3] * 4, "4": [4] * 3, "6": [6] * 2, "12": [12], "5+7": [5, 7]}


def check_rows(rows, pcm, rep, rec, what):
    """a run's PCM [NSLOTS][ns][2304], reports and records against the oracle: every sample a fed stream's slots hold, every record word;
    POISON wherever a feed does not write"""
    for s, r in enumerate(rows):
        if r["fcfg"] is None:
            assert (pcm[:, s] == POISON).all() and (rep["status"][:, s] == D.EMPTY).all(), (what, r["name"])
            assert rec[s] == np.zeros((), dtype=RECORD_DTYPE)
            continue
        n = 1152 * r["fcfg"]["channels"]
        assert [bool(x & LOST_BITS) for x in rep["status"][:, s]] == r["lost"], (what, r["case"], r["name"])
        want_pcm, want_rec = oracle_of(r)
        assert (pcm[:, s, n:] == POISON).all(), (what, r["case"], r["name"])
        bad = np.nonzero((pcm[:, s, :n] != want_pcm[:, :n]).any(axis=1))[0]
        assert bad.size == 0, (what, r["case"], r["name"], "slots", bad.tolist())
        assert rec[s] == want_rec, (what, r["case"], r["name"], rec[s], want_rec)


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation (tests/emu/mp2_conceal_emu.cpp) and its sanitizer driver (tests/emu/mp2_conceal_san_main.cpp)
_SRC = [str(ROOT / "tests" / "emu" / "mp2_conceal_emu.cpp"), str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp")]


def build_emu(outdir):
    so = Path(outdir) / "libmp2concealemu.so"
    subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + F._FLAGS + ["-o", str(so)] + _SRC + ["-lm"], check=True)
    return so


def build_san_driver(outdir):
    """the driver + the emulation + csrc/mp2_host.cpp as ONE program under AddressSanitizer + UBSan (linked, not preloaded)"""
    exe = Path(outdir) / "mp2_conceal_san"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + F._FLAGS + ["-o", str(exe),
                    str(ROOT / "tests" / "emu" / "mp2_conceal_san_main.cpp")] + _SRC + ["-lm"], check=True)
    return exe


def _cfg_arrays(rows):
    n = len(rows)
    fs = (C.c_long * n)(*[r["fcfg"]["samplerate"] if r["fcfg"] else 0 for r in rows])
    kb = (C.c_int * n)(*[r["fcfg"]["bitrate"] if r["fcfg"] else 0 for r in rows])
    ch = (C.c_int * n)(*[r["fcfg"]["channels"] if r["fcfg"] else 0 for r in rows])
    ho = (C.c_int * n)(*[r["hold"] for r in rows])
    st = (C.c_int * n)(*[r["step"] for r in rows])
    return fs, kb, ch, ho, st


class ConcealEmu:
    """N streams on the emulated feed path with concealment; rows: dicts with fcfg (None: no feed), hold (0: off) and step.  decode()
    mirrors tlb_feed_host with an output buffer that holds POISON before the call."""

    def __init__(self, so, rows):
        L = self.L = C.CDLL(str(so))
        L.conceal_create.restype = C.c_void_p
        L.conceal_create.argtypes = [C.c_int] + [C.c_void_p] * 6
        L.conceal_destroy.argtypes = [C.c_void_p]
        L.conceal_stride.argtypes = [C.c_void_p]
        L.conceal_reset.argtypes = [C.c_void_p, C.c_int]
        L.conceal_records.argtypes = [C.c_void_p, C.c_void_p]
        L.conceal_guard_ok.argtypes = [C.c_void_p]
        L.conceal_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert L.conceal_sizeof_report() == F.REPORT_DTYPE.itemsize
        self.n = len(rows)
        err = C.c_int(0)
        self.h = L.conceal_create(self.n, *_cfg_arrays(rows), C.byref(err))
        assert self.h, err.value
        self.stride = L.conceal_stride(self.h)

    def decode(self, frames, lens):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        assert frames.shape == (nf, self.n, self.stride)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        rep = np.zeros((nf, self.n), dtype=F.REPORT_DTYPE)
        pcm = np.full((nf, self.n, 2304), POISON, dtype=np.int16)
        rc = self.L.conceal_decode(self.h, frames.ctypes.data, ln.ctypes.data, nf, pcm.ctypes.data, rep.ctypes.data)
        assert rc == 0, rc
        return pcm, rep

    def run_cut(self, frames, lens, cut):
        """the slots in calls of cut[0], cut[1], ... -> (pcm, reports, records) of the whole run"""
        at, pcm, rep = 0, [], []
        for n in cut:
            p, r = self.decode(frames[at:at + n], lens[at:at + n])
            pcm.append(p); rep.append(r)
            at += n
        assert at == frames.shape[0]
        return np.concatenate(pcm), np.concatenate(rep), self.records()

    def records(self):
        rec = np.zeros(self.n, dtype=RECORD_DTYPE)
        self.L.conceal_records(self.h, rec.ctypes.data)
        return rec

    def guard_ok(self):
        return bool(self.L.conceal_guard_ok(self.h))

    def reset(self, s=-1):
        assert self.L.conceal_reset(self.h, s) == 0

    def close(self):
        if self.h:
            self.L.conceal_destroy(self.h)
            self.h = None


def emu_fold(so, hold, step, status, cut):
    """the carry alone over a hand-written status sequence -> its record"""
    L = C.CDLL(str(so))
    L.conceal_fold.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    st = np.ascontiguousarray(status, dtype=np.uint32)
    ct = np.ascontiguousarray(cut, dtype=np.int32)
    rec = np.zeros((), dtype=RECORD_DTYPE)
    rc = L.conceal_fold(hold, step, st.ctypes.data, st.size, ct.ctypes.data, ct.size, rec.ctypes.data)
    assert rc == 0, rc
    return rec


def run_san_driver(exe, workdir, rows, calls):
    """calls: [(frames, lens)] of ONE run from the reset -> ([(report, pcm)] per call, records, guard flag) as the sanitized program wrote them"""
    fin, fout = Path(workdir) / "conceal_cases.bin", Path(workdir) / "conceal_results.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ii", len(rows), len(calls)))
        for r in rows:
            c = r["fcfg"]
            f.write(struct.pack("<qiiii", c["samplerate"] if c else 0, c["bitrate"] if c else 0, c["channels"] if c else 0, r["hold"], r["step"]))
        for fr, ln in calls:
            f.write(struct.pack("<i", fr.shape[0]))
            f.write(np.ascontiguousarray(fr, dtype=np.uint8).tobytes())
            f.write(np.ascontiguousarray(ln, dtype=np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    blob, pos, out = fout.read_bytes(), 0, []
    ns = len(rows)
    for fr, _ in calls:
        nf, one = fr.shape[0], []
        for dt, shape in ((F.REPORT_DTYPE, (nf, ns)), (np.dtype(np.int16), (nf, ns, 2304))):
            n = dt.itemsize * int(np.prod(shape))
            one.append(np.frombuffer(blob[pos:pos + n], dtype=dt).reshape(shape))
            pos += n
        out.append(tuple(one))
    rec = np.frombuffer(blob[pos:pos + 32 * ns], dtype=RECORD_DTYPE)
    pos += 32 * ns
    guard, = struct.unpack("<i", blob[pos:pos + 4])
    assert pos + 4 == len(blob)
    return out, rec, bool(guard)
