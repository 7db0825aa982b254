"""Support for the adapted-feed tests (test_feed_adapt_*.py): the schedule's closed form in Python ints, the numpy oracle -- feedlib's decode
of the WANTED frames, the channel map, resamplelib's formula, cut into ticks; it shares no code with the emulation --, the emulation of the
kernels through feedlib (tests/emu/mp2_feed_emu.cpp, the one feed emulation), and the stream set and inputs the test files share.
A plain module: nothing here is collected by pytest."""
import ctypes as C
import tempfile

import numpy as np

import declib as D
import feedlib as F
import resamplelib as R

ROOT = F.ROOT
N = 1152
POISON = F.POISON
UNWANTED = 0x100
NTICKS = 14                                                          # 160/147: past the first unwanted tick (12) and the five-tick need cycle; thirteen feed frames
CUTS = ((14,), (1, 5, 8), (1,) * 14)
# the stream set: feed (rate, mode of the source encoder, kbps, pcmgen kind) or None, the stream's (rate, mode), set through the adapted entry
STREAMS = [dict(feed=(44100, "s", 128, 5), enc=(48000, "s"), adapt=True),
           dict(feed=(32000, "s", 128, 7), enc=(48000, "m"), adapt=True),        # map + resample
           dict(feed=(22050, "m", 32, 0), enc=(24000, "s"), adapt=True),
           dict(feed=(16000, "s", 64, 2), enc=(24000, "s"), adapt=True),
           dict(feed=(48000, "s", 128, 0), enc=(48000, "m"), adapt=True),        # 1/1, two channels to one
           dict(feed=(48000, "m", 64, 4), enc=(48000, "s"), adapt=True),         # 1/1, one channel to two
           dict(feed=(48000, "s", 192, 3), enc=(48000, "s"), adapt=False),       # a strict feed beside them
           dict(feed=None, enc=(48000, "s"), adapt=False)]                       # and a stream without a feed


def ratio_of(fs, es):
    """(L, M); (1, 1) for equal rates; None: no legal pair"""
    return (1, 1) if fs == es else R.ratio_of(fs, es)


def S(f, L, M):
    return (N * f - 1) * M // L + 1 if f > 0 else 0


def K(f, L, M):
    return -(-S(f + 1, L, M) // N) if f >= 0 else 0


def want(f, L, M):
    return K(f, L, M) - K(f - 1, L, M)


def fcfg_of(st):
    return F.feed_cfg_of(st["feed"]) if st["feed"] else None


def enc_nch(st):
    return 1 if st["enc"][1] == "m" else 2


def lm_of(st):
    return ratio_of(st["feed"][0], st["enc"][0])


_frames = {}


def feed_frames(i, st, n=NTICKS):
    """the oracle encoder's `n` frames of stream i's feed (CPU), once per process"""
    key = (i, st["feed"], n)
    if key not in _frames:
        _frames[key] = F.oracle_frames(st["feed"], F.case_pcm(40 + i, st["feed"], n))
    return _frames[key]


def slots_on_schedule(streams, nticks=NTICKS):
    """per stream a list of (bytes, len) per tick: the next feed frame on a wanted tick, an empty slot on an unwanted one (and for a stream
    without a feed) -> (slot lists, per stream the frames in wanted order)"""
    lists, used = [], []
    for i, st in enumerate(streams):
        if not st["feed"]:
            lists.append([(b"", 0)] * nticks); used.append([])
            continue
        fr = feed_frames(i, st)
        L, M = lm_of(st)
        sl, k = [], 0
        for f in range(nticks):
            if want(f, L, M):
                sl.append((fr[k], len(fr[k]))); k += 1
            else:
                sl.append((b"", 0))
        lists.append(sl); used.append(list(fr[:k]))
    return lists, used


def channel_map(x, fch, sch):
    """x int [n][fch] -> [n][the resampler's channels]: two to one is (L + R + 1) >> 1; one to two stays one (the OUTPUT goes to both)"""
    x = np.asarray(x, dtype=np.int64)
    if fch == 2 and sch == 1:
        return ((x[:, 0] + x[:, 1] + 1) >> 1)[:, None]
    return x


def oracle_ticks(x, fs, es, fch, sch, nticks):
    """x int [source frames since the reset][fch] -> int16 [nticks][2304] as the ingest reads it (zeros where nothing is written)"""
    xm = channel_map(x, fch, sch)
    if fs == es:
        y = xm[:N * nticks]
    else:
        y = R.oracle_stream(xm, fs, es, N * nticks)
    if fch == 1 and sch == 2:
        y = np.repeat(y, 2, axis=1)
    out = np.zeros((nticks, 2 * N), dtype=np.int16)
    out[:, :N * sch] = y.astype(np.int16).reshape(nticks, N * sch)
    return out


def oracle_pcm(frames, st, nticks=NTICKS):
    """frames: the stream's WANTED slots in order (bytes, or None for a slot that decodes to silence) -> int16 [nticks][2304]"""
    fc = fcfg_of(st)
    fch = fc["channels"]
    d = F.numpy_feed_pcm(frames, fc)[:, :N * fch].reshape(-1, fch)
    return oracle_ticks(d, st["feed"][0], st["enc"][0], fch, enc_nch(st), nticks)


def written(streams, nticks):
    """bool [nticks][ns][2304]: what a feed call writes: the first 1152 * channels of the STREAM for an adapted feed, of the FEED for a strict one"""
    m = np.zeros((nticks, len(streams), 2 * N), dtype=bool)
    for s, st in enumerate(streams):
        if st["feed"]:
            m[:, s, :N * enc_nch(st)] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation, the sanitizer driver and the ctypes layer are feedlib's; here: a stream set as feedlib's rows, the calls cut by cut
_emu_so = None


def rows_of(streams):
    return [(fcfg_of(st), int(st["adapt"]), st["enc"][0], enc_nch(st)) for st in streams]


def build_emu():
    """feedlib.build_emu into a temporary directory, once per process"""
    global _emu_so
    if _emu_so is None:
        _emu_so = F.build_emu(tempfile.mkdtemp(prefix="faemu"))
    return _emu_so


build_san_driver = F.build_san_driver


def run_san_driver(exe, workdir, streams, cases):
    """cases: [[(frames, lens), ...]]: per case the calls of one run from the reset -> per case (report, pcm) over all its ticks, as the
    sanitized program wrote them (every sample POISON before each call)"""
    return [(np.concatenate([r for r, _ in calls]), np.concatenate([p for _, p in calls])) for calls in F.run_san_rows(exe, workdir, rows_of(streams), cases)]


class FeedAdaptEmu(F.FeedEmu):
    """a stream set on the emulated strict + adapted feed path; decode() mirrors tlb_feed_host with an output buffer that holds POISON"""

    def __init__(self, streams):
        super().__init__(build_emu(), None, rows_of(streams))

    def run_cuts(self, frames, lens, cuts):
        """the ticks of (frames, lens) call by call -> (pcm, report) over all of them"""
        out, f0 = [], 0
        for n in cuts:
            out.append(self.decode(frames[f0:f0 + n], lens[f0:f0 + n]))
            f0 += n
        return np.concatenate([p for p, _ in out]), np.concatenate([r for _, r in out])


def resample_plane(fs, es, fch, sch, x, nticks):
    """the emulation's resample stage alone over a source plane x int16 [>= K(nticks - 1) * 1152][fch] -> int16 [nticks][2304] (POISON where nothing is written)"""
    L = C.CDLL(str(build_emu()))
    L.feed_resample_plane.argtypes = [C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    x = np.ascontiguousarray(x, dtype=np.int16)
    out = np.full((nticks, 2 * N), POISON, dtype=np.int16)
    rc = L.feed_resample_plane(fs, es, fch, sch, x.ctypes.data, nticks, out.ctypes.data)
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
_shared = {}


def shared():
    """the stream set's inputs and oracle, once per process: frames / lens [NTICKS][ns][stride], `used` the frames in wanted order,
    `want` the oracle's PCM [NTICKS][ns][2304] (zeros for the stream without a feed and where nothing is written)"""
    if not _shared:
        lists, used = slots_on_schedule(STREAMS)
        stride = max(F.slot_bytes(fcfg_of(st)) for st in STREAMS if st["feed"])
        fr, ln = F.slots_to_arrays(lists, stride)
        wantp = np.zeros((NTICKS, len(STREAMS), 2 * N), dtype=np.int16)
        for s, st in enumerate(STREAMS):
            if st["feed"]:
                wantp[:, s] = oracle_pcm(used[s], st)
        _shared.update(lists=lists, used=used, stride=stride, fr=fr, ln=ln, want=wantp)
    return _shared


def stream_configs(streams=STREAMS, psy=1):
    import odr_audioenc_amd as M
    return [M.StreamConfig(samplerate=st["enc"][0], mode=st["enc"][1], bitrate=(128 if st["enc"][0] == 48000 else 64) if st["enc"][1] != "m" else 64, psy_model=psy) for st in streams]


def set_feeds(obj, streams=STREAMS):
    """the set's feeds on a Batch, Tick or Node"""
    import odr_audioenc_amd as M
    for s, st in enumerate(streams):
        if st["feed"]:
            c = fcfg_of(st)
            obj.set_feed(s, M.FeedConfig(samplerate=c["samplerate"], bitrate=c["bitrate"], channels=c["channels"]), adapt=st["adapt"])
