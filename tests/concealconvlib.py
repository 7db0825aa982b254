"""Support for the tests of the feed concealment on ADAPTED and DOWN feeds (test_conceal_conv_*.py; csrc/mp2_conceal_conv.h).  The ORACLE
composes what exists and shares no code with the kernels: conceallib.oracle_stream over a stream's WANTED slots at the feed's own
configuration, then the channel map and formula of feedadaptlib / resamplelib, or of feeddownlib / decimatelib -- the chain "strict
concealed feed, map, resampler or decimator" the feature is defined by.  Here too: the seven feed cases, the scenarios (conceallib's, made
longer, plus the ones only a schedule with unwanted slots has), their placement on the wanted slots of a schedule, the cuts in ticks, and
the emulation (tests/emu/mp2_conceal_conv_emu.cpp) with its ctypes layer and its sanitizer driver.  A plain module: nothing here is
collected by pytest."""
import ctypes as C
import os
import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import conceallib as K
import declib as D
import feedadaptlib as FA
import feeddownlib as FD
import feedlib as F

ROOT = F.ROOT
N = 1152
POISON = F.POISON
UNWANTED = 0x100
RECORD_DTYPE = K.RECORD_DTYPE
NW_MIN = 16                                                          # wanted slots per stream, at least: conceallib's twelve and a tail (23 ticks at 3/2)
# kind, feed (rate, mode of the source encoder, kbps, pcmgen kind), the stream's (rate, mode)
CASES = [("adapt", (32000, "s", 128, 7), (48000, "s")),
         ("adapt", (44100, "s", 128, 5), (48000, "m")),              # map + resample; the first unwanted tick is tick 12
         ("adapt", (48000, "m", 64, 4), (48000, "s")),               # ratio 1/1, one channel to two
         ("adapt", (16000, "s", 64, 2), (24000, "s")),
         ("down", (48000, "s", 192, 0), (24000, "s")),               # every tick wants two
         ("down", (32000, "s", 128, 7), (24000, "s")),               # the first one-frame tick is tick 1
         ("down", (44100, "m", 64, 4), (24000, "m"))]                # ... is tick 6
CASE_IDS = ["%s_%dk%s_to_%dk%s" % (k, f[0] // 1000, f[1], e[0] // 1000, e[1]) for k, f, e in CASES]


# ---------------------------------------------------------------------------------------------------------------------------------
# the schedule of a case: per tick how many slots are wanted (feedadaptlib / feeddownlib restate the closed forms)
def slots_per_tick(case):
    return 2 if case[0] == "down" else 1


def feed_want_at(case, tick):
    """wanted slots of tick `tick` counted from the stream's reset"""
    kind, feed, enc = case
    if kind == "down":
        return FD.want(tick, *FD.RATIOS[feed[0]])
    return FA.want(tick, *FA.ratio_of(feed[0], enc[0]))


down_feed_want_at = feed_want_at


def schedule(case):
    """-> (nticks, nw, want per tick): the fewest whole ticks with at least NW_MIN wanted slots"""
    w, nt = [], 0
    while sum(w) < NW_MIN:
        w.append(feed_want_at(case, nt)); nt += 1
    return nt, sum(w), w


def first_short_tick(case):
    """the first tick with an unwanted slot that has at least four wanted slots before it (a loss run ahead of it then has a G), and
    their number; (None, 8) for a schedule without unwanted slots"""
    nt, _, w = schedule(case)
    for t in range(nt):
        if w[t] < slots_per_tick(case) and sum(w[:t + 1]) >= 4:
            return t, sum(w[:t + 1])
    return None, 8


def enc_nch(case):
    return 1 if case[2][1] == "m" else 2


def fcfg_of(case):
    return F.feed_cfg_of(case[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenarios over nw wanted slots: (name, hold, step, ways per wanted slot, fill) -- fill: the unwanted slots carry a good frame's bytes
TAIL = [None, "crc", "empty", None]


def scenarios(case):
    nt, nw, _ = schedule(case)
    out = []
    for name, hold, step, ways in K.scenarios(long_ok=False):        # (a case's slots are as wide as its own frames: no room for a slot longer than its frame)
        out.append((name, hold, step, (list(ways) + TAIL + [None] * nw)[:nw], False))
    _, a = first_short_tick(case)                                # an unwanted slot lies between wanted slots a - 1 and a

    def run(first, n):
        return ["empty" if first <= i < first + n else None for i in range(nw)]
    out.append(("inside", 4, 3, run(a - 2, 4), True))            # ... INSIDE a loss run, and it carries bytes: nothing may change
    out.append(("behind", 4, 3, run(a - 3, 3), False))           # ... directly BEHIND one
    out.append(("even", 4, 3, ["sync" if i % 2 == 0 else None for i in range(nw)], True))     # a down feed's slot 0 lost and slot 1 not ("alternating": the other way)
    return out


_FRAMES = {}


def case_frames(ci):
    """the oracle encoder's frames of case ci (CPU), once: one per wanted slot"""
    if ci not in _FRAMES:
        feed = CASES[ci][1]
        _FRAMES[ci] = F.oracle_frames(feed, F.case_pcm(80 + ci, feed, schedule(CASES[ci])[1]))
    return _FRAMES[ci]


def place(case, wanted, fill=None):
    """a stream's wanted slots [(bytes, len)] on the schedule from a reset -> per tick one (bytes, len), or two for a down feed; an unwanted
    slot is empty, or carries `fill`"""
    nt, nw, w = schedule(case)
    assert len(wanted) == nw
    per, k, out = slots_per_tick(case), 0, []
    other = (b"", 0) if fill is None else (fill, len(fill))
    for t in range(nt):
        tick = [wanted[k + j] if j < w[t] else other for j in range(per)]
        k += w[t]
        out.append(tick if per == 2 else tick[0])
    return out


def scenario_batch(ci, names=None):
    """every scenario of case ci (or the named ones) as one stream each, then a fed stream WITHOUT concealment (the "ways" losses) and a
    stream without a feed -> list of dict(ci, name, fcfg, enc_rate, enc_nch, w, hold, step, wanted, lost, ticks, fill); w: wanted slots per tick"""
    case = CASES[ci]
    fcfg, frames = fcfg_of(case), case_frames(ci)
    nt, nw, w = schedule(case)
    enc = dict(ci=ci, enc_rate=case[2][0], enc_nch=enc_nch(case), w=w)
    rows = []
    sc = scenarios(case)
    for name, hold, step, ways, fill in sc + [("unconcealed", 0, 0, sc[8][3], False)]:
        if names is not None and name not in names:
            continue
        wanted = K.slots_of(frames, ways, fcfg)
        rows.append(dict(enc, name=name, fcfg=fcfg, hold=hold, step=step, wanted=wanted, lost=[x is not None for x in ways],
                         ticks=place(case, wanted, frames[0] if fill else None), fill=fill))
    empty = (b"", 0)
    rows.append(dict(enc, name="unfed", fcfg=None, hold=0, step=0, wanted=[], lost=[], ticks=[[empty, empty] if slots_per_tick(case) == 2 else empty] * nt, fill=False))
    return rows


def multi_batch(cis, names):
    """the named scenarios of several cases of ONE kind as one batch: every stream's ticks made as many as the longest case's, with empty
    ticks behind its own -- whose wanted slots are lost ones of its sequence"""
    assert len({CASES[ci][0] for ci in cis}) == 1
    rows = [r for ci in cis for r in scenario_batch(ci, names)]
    nt = max(len(r["ticks"]) for r in rows)
    empty = (b"", 0)
    for r in rows:
        case = CASES[r["ci"]]
        more = [feed_want_at(case, t) for t in range(len(r["ticks"]), nt)]
        r["ticks"] = list(r["ticks"]) + [[empty, empty] if slots_per_tick(case) == 2 else empty] * len(more)
        if r["fcfg"]:
            r["w"] = list(r["w"]) + more
            r["wanted"] = list(r["wanted"]) + [empty] * sum(more)
            r["lost"] = list(r["lost"]) + [True] * sum(more)
    return rows


def kind_of(rows):
    return CASES[rows[0]["ci"]][0]


def batch_arrays(rows, stride):
    lists = [r["ticks"] for r in rows]
    return FD.slots_to_arrays(lists, stride) if kind_of(rows) == "down" else F.slots_to_arrays(lists, stride)


def cuts_of(case):
    """conceallib.CUTS as cuts of this case's ticks (each cut's sizes over and over), and one with a call boundary either side of the first
    tick that has an unwanted slot"""
    nt = schedule(case)[0]
    out = {}
    for name, sizes in K.CUTS.items():
        cut, i = [], 0
        while sum(cut) < nt:
            cut.append(min(sizes[i % len(sizes)], nt - sum(cut))); i += 1
        out[name] = cut
    u, _ = first_short_tick(case)
    if u is not None:
        out["unwanted"] = [n for n in (u, 1, nt - u - 1) if n > 0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle: the chain, in numpy
_ORACLE = {}


def oracle_of(row):
    """(pcm int16 [nticks][2304] as the ingest reads it, record) of a scenario row, once (do not write to it)"""
    ci = row["ci"]
    key = (ci, row["name"], len(row["w"]))
    if key not in _ORACLE:
        case = CASES[ci]
        kind, feed, enc = case
        fcfg, nt = row["fcfg"], len(row["w"])
        fch = fcfg["channels"]
        if row["hold"]:
            src, rec = K.oracle_stream(row["wanted"], row["lost"], fcfg, row["hold"], row["step"])
        else:
            src = F.numpy_feed_pcm([None if gone else bytes(b)[:n] for (b, n), gone in zip(row["wanted"], row["lost"])], fcfg)
            rec = np.zeros((), dtype=RECORD_DTYPE)
        x = src[:, :N * fch].reshape(-1, fch)
        pcm = FD.oracle_ticks(x, feed[0], fch, enc_nch(case), nt) if kind == "down" else FA.oracle_ticks(x, feed[0], enc[0], fch, enc_nch(case), nt)
        pcm.setflags(write=False)
        _ORACLE[key] = (pcm, rec)
    return _ORACLE[key]


def check_rows(rows, pcm, rep, rec, what):
    """a run's PCM [nticks][ns][2304], reports ([nticks][ns] or [nticks][ns][2]) and records against the oracle: every sample the stream's
    slots hold over its own ticks, every record word, every report's lost bit and the unwanted slots' status; POISON wherever a feed does
    not write"""
    per = 2 if kind_of(rows) == "down" else 1
    st = rep["status"].reshape(pcm.shape[0], len(rows), per)
    for s, r in enumerate(rows):
        ci = r["ci"]
        case = CASES[ci]
        w = r["w"]
        nt = len(w)
        if r["fcfg"] is None:
            assert (pcm[:, s] == POISON).all() and (st[:, s] == D.EMPTY).all(), (what, r["name"])
            assert rec[s] == np.zeros((), dtype=RECORD_DTYPE)
            continue
        got = [bool(st[t, s, j] & K.LOST_BITS) for t in range(nt) for j in range(w[t])]
        assert got == r["lost"], (what, r["name"])
        other = [int(st[t, s, j]) for t in range(nt) for j in range(w[t], per)]
        assert other == [D.EMPTY | (UNWANTED if r["fill"] else 0)] * len(other), (what, r["name"], other)
        want_pcm, want_rec = oracle_of(r)
        n = N * enc_nch(case)
        assert (pcm[:, s, n:] == POISON).all(), (what, r["name"])
        assert nt == pcm.shape[0]
        bad = np.nonzero((pcm[:, s, :n] != want_pcm[:, :n]).any(axis=1))[0]
        assert bad.size == 0, (what, CASE_IDS[ci], r["name"], "ticks", bad.tolist())
        assert rec[s] == want_rec, (what, CASE_IDS[ci], r["name"], rec[s], want_rec)


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation (tests/emu/mp2_conceal_conv_emu.cpp) and its sanitizer driver (tests/emu/mp2_conceal_conv_san_main.cpp)
_SRC = [str(ROOT / "tests" / "emu" / "mp2_conceal_conv_emu.cpp"), str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp")]
_built = {}


def build_emu():
    if "so" not in _built:
        so = Path(tempfile.mkdtemp(prefix="ccvemu")) / "libmp2concealconvemu.so"
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + F._FLAGS + ["-o", str(so)] + _SRC + ["-lm"], check=True)
        _built["so"] = so
    return _built["so"]


def build_san_driver():
    """the driver + the emulation + csrc/mp2_host.cpp as ONE program under AddressSanitizer + UBSan (linked, not preloaded)"""
    if "san" not in _built:
        exe = Path(tempfile.mkdtemp(prefix="ccvsan")) / "mp2_conceal_conv_san"
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + F._FLAGS + ["-o", str(exe),
                        str(ROOT / "tests" / "emu" / "mp2_conceal_conv_san_main.cpp")] + _SRC + ["-lm"], check=True)
        _built["san"] = exe
    return _built["san"]


class ConcealConvEmu:
    """the streams of one case on the emulated adapted or down path with concealment; rows: dicts with fcfg (None: no feed), hold (0: off)
    and step.  decode() mirrors tlb_feed_host / tlb_feed_down_host with an output buffer that holds POISON before the call."""

    def __init__(self, rows):
        L = self.L = C.CDLL(str(build_emu()))
        L.ccv_create.restype = C.c_void_p
        L.ccv_create.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8
        L.ccv_destroy.argtypes = [C.c_void_p]
        L.ccv_stride.argtypes = [C.c_void_p]
        L.ccv_reset.argtypes = [C.c_void_p, C.c_int]
        L.ccv_records.argtypes = [C.c_void_p, C.c_void_p]
        L.ccv_guard_ok.argtypes = [C.c_void_p]
        L.ccv_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert L.ccv_sizeof_report() == F.REPORT_DTYPE.itemsize
        n = self.n = len(rows)
        self.per = 2 if kind_of(rows) == "down" else 1
        fs = (C.c_long * n)(*[r["fcfg"]["samplerate"] if r["fcfg"] else 0 for r in rows])
        kb = (C.c_int * n)(*[r["fcfg"]["bitrate"] if r["fcfg"] else 0 for r in rows])
        ch = (C.c_int * n)(*[r["fcfg"]["channels"] if r["fcfg"] else 0 for r in rows])
        er = (C.c_long * n)(*[r["enc_rate"] for r in rows])
        en = (C.c_int * n)(*[r["enc_nch"] for r in rows])
        ho = (C.c_int * n)(*[r["hold"] for r in rows])
        st = (C.c_int * n)(*[r["step"] for r in rows])
        err = C.c_int(0)
        self.h = L.ccv_create(self.per - 1, n, fs, kb, ch, er, en, ho, st, C.byref(err))
        assert self.h, err.value
        self.stride = L.ccv_stride(self.h)

    def decode(self, frames, lens):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        shape = (nf, self.n, 2) if self.per == 2 else (nf, self.n)
        assert frames.shape == shape + (self.stride,)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        assert ln.shape == shape
        rep = np.zeros(shape, dtype=F.REPORT_DTYPE)
        pcm = np.full((nf, self.n, 2304), POISON, dtype=np.int16)
        rc = self.L.ccv_decode(self.h, frames.ctypes.data, ln.ctypes.data, nf, pcm.ctypes.data, rep.ctypes.data)
        assert rc == 0, rc
        return pcm, rep

    def run_cut(self, frames, lens, cut):
        """the ticks in calls of cut[0], cut[1], ... -> (pcm, reports, records) of the whole run"""
        at, pcm, rep = 0, [], []
        for n in cut:
            p, r = self.decode(frames[at:at + n], lens[at:at + n])
            pcm.append(p); rep.append(r)
            at += n
        assert at == frames.shape[0]
        return np.concatenate(pcm), np.concatenate(rep), self.records()

    def records(self):
        rec = np.zeros(self.n, dtype=RECORD_DTYPE)
        self.L.ccv_records(self.h, rec.ctypes.data)
        return rec

    def guard_ok(self):
        return bool(self.L.ccv_guard_ok(self.h))

    def reset(self, s=-1):
        assert self.L.ccv_reset(self.h, s) == 0

    def close(self):
        if self.h:
            self.L.ccv_destroy(self.h)
            self.h = None


def run_san_driver(exe, workdir, rows, calls):
    """calls: [(frames, lens)] of ONE run from the reset -> ([(report, pcm)] per call, records, guard flag) as the sanitized program wrote them"""
    fin, fout = Path(workdir) / "ccv_cases.bin", Path(workdir) / "ccv_results.bin"
    per = 2 if kind_of(rows) == "down" else 1
    with open(fin, "wb") as f:
        f.write(struct.pack("<iii", per - 1, len(rows), len(calls)))
        for r in rows:
            c = r["fcfg"]
            f.write(struct.pack("<qiiiiqi", c["samplerate"] if c else 0, c["bitrate"] if c else 0, c["channels"] if c else 0, r["hold"], r["step"], r["enc_rate"], r["enc_nch"]))
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
        for dt, shape in ((F.REPORT_DTYPE, (nf, ns, 2) if per == 2 else (nf, ns)), (np.dtype(np.int16), (nf, ns, 2304))):
            n = dt.itemsize * int(np.prod(shape))
            one.append(np.frombuffer(blob[pos:pos + n], dtype=dt).reshape(shape))
            pos += n
        out.append(tuple(one))
    rec = np.frombuffer(blob[pos:pos + 32 * ns], dtype=RECORD_DTYPE)
    pos += 32 * ns
    guard, = struct.unpack("<i", blob[pos:pos + 4])
    assert pos + 4 == len(blob)
    return out, rec, bool(guard)
