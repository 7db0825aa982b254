"""The feed concealment's C-ABI.  Without a GPU: the header declares exactly the tlb_*conceal* names and the library exports each, the record
is 32 bytes with the field offsets of the binding's dtype, the NULL-handle calls answer without touching a device.  On a GPU (a batch
cannot be made without one): every refusal of tlb_conceal_enable with nothing changed afterwards, the all-or-nothing check of stream -1,
enable / get / disable, and what tlb_feed_set and tlb_feed_reset do to the state."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "toolame_batch.h"
NAMES = ["tlb_conceal_enable", "tlb_conceal_get", "tlb_conceal_reset", "tlb_conceal_records_device", "tlb_conceal_records_host",
         "tlb_tick_enable_conceal", "tlb_tick_conceal", "tlb_tick_conceal_reset",
         "tlb_node_enable_conceal", "tlb_node_conceal", "tlb_node_conceal_reset"]
OTHERS = ("monitor", "compare", "feed", "resample", "decimate", "decode", "loudness", "truepeak", "limiter")      # words whose own ABI tests claim every name that contains them
ARG = 18


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_header_declares_and_library_exports_exactly_the_names(M):
    src = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]*conceal[a-z0-9_]*)\s*\(", src))
    assert declared == set(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {n for n in exported if "conceal" in n} == set(NAMES)
    assert not [n for n in NAMES for w in OTHERS if w in n]
    assert re.search(r"#define TLB_CONCEAL_MAX_HOLD 16\b", src) and re.search(r"#define TLB_CONCEAL_MAX_STEP 21\b", src)
    assert M.CONCEAL_MUTE == 0xFFFFFFFF and re.search(r"#define TLB_CONCEAL_MUTE 0xFFFFFFFFu", src)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_record_is_32_bytes_with_the_offsets_of_the_dtype(M, tmp_path):
    ctype, dt = "tlb_conceal_record", M.CONCEAL_DTYPE
    fields = list(dt.names)
    assert fields == ["frames", "passed", "concealed", "muted", "runs", "longest", "run", "offset"]
    prog = tmp_path / (ctype + ".c")
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "toolame_batch.h"\nint main(void) {\n    printf("%%zu", sizeof(%s));\n' % ctype
                    + "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / ctype
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 32 == dt.itemsize
    assert got[1:] == [dt.fields[f][1] for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28]


def test_null_handles_answer_without_a_gpu(M):
    import ctypes as C
    L = M.load_library()
    rec = np.zeros(4, dtype=M.CONCEAL_DTYPE)
    hold, step = C.c_int(7), C.c_int(7)
    assert L.tlb_conceal_enable(None, -1, 4, 3) == ARG and L.tlb_conceal_reset(None, -1) == ARG
    assert L.tlb_conceal_get(None, 0, C.byref(hold), C.byref(step)) == -ARG and (hold.value, step.value) == (7, 7)
    assert L.tlb_conceal_records_device(None, rec.ctypes.data, None) == ARG and L.tlb_conceal_records_host(None, rec.ctypes.data) == ARG
    assert L.tlb_tick_enable_conceal(None, -1, 4, 3) == ARG and L.tlb_tick_conceal_reset(None, 0) == ARG
    assert L.tlb_node_enable_conceal(None, -1, 4, 3) == ARG and L.tlb_node_conceal_reset(None, -1) == ARG
    assert L.tlb_tick_conceal(None) is None and L.tlb_node_conceal(None, 0) is None
    assert not rec.view(np.uint8).any()


# ---- with a batch ----------------------------------------------------------------------------------------------------------------------
def _scfg(M, fs, mode, kbps):
    return M.StreamConfig(samplerate=fs, mode=mode, bitrate=kbps, psy_model=1, pad_len=0)


def _batch(M):
    """five streams: 0, 1 strict feeds (48 kHz stereo 192), 2 an adapted feed (32 kHz into 48 kHz), 3 a down feed (48 kHz into 24 kHz), 4 no feed"""
    b = M.Batch([_scfg(M, 48000, "s", 128)] * 3 + [_scfg(M, 24000, "s", 64), _scfg(M, 48000, "s", 128)])
    fc = M.FeedConfig(48000, 192, 2)
    b.set_feed(0, fc); b.set_feed(1, fc)
    b.set_feed(2, M.FeedConfig(32000, 128, 2), adapt=True)
    b.set_down_feed(3, fc)
    return b, fc


def _code(M, fn, *a, **kw):
    with pytest.raises(M.ToolameError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.gpu
def test_every_refusal_changes_nothing(M):
    b, _ = _batch(M)
    assert all(b.conceal_cfg(s) is None for s in range(5))
    assert _code(M, b.conceal_records) == ARG                    # never enabled: no records
    b.conceal_reset()                                            # ... and nothing to forget
    b.enable_conceal(0, 3)                                       # off on a batch that never had it on: nothing happens
    assert _code(M, b.conceal_records) == ARG
    refusals = [dict(stream=4), dict(stream=2), dict(stream=3), dict(stream=0, hold=17), dict(stream=0, hold=-1), dict(stream=0, step=0),
                dict(stream=0, step=22), dict(stream=5), dict(stream=-2), dict(stream=-1)]
    for kw in refusals:                                          # no strict feed; adapted; down; hold; step; no such stream; all: some stream has none
        assert _code(M, b.enable_conceal, **kw) == ARG, kw
        assert all(b.conceal_cfg(s) is None for s in range(5)), kw
        assert _code(M, b.conceal_records) == ARG, kw            # nothing was allocated either
    b.enable_conceal(4, 3, stream=0)
    for kw in refusals:                                          # ... and the same with concealment on for one stream: it keeps what it has
        assert _code(M, b.enable_conceal, **kw) == ARG, kw
        assert [b.conceal_cfg(s) for s in range(5)] == [(4, 3), None, None, None, None], kw
    assert _code(M, b.conceal_cfg, 5) == ARG and _code(M, b.conceal_reset, 5) == ARG
    b.close()


@pytest.mark.gpu
def test_enable_get_disable_and_the_all_or_nothing_of_every_stream(M):
    b, fc = _batch(M)
    b.enable_conceal(16, 21, stream=1)
    assert [b.conceal_cfg(s) for s in range(5)] == [None, (16, 21), None, None, None]
    assert _code(M, b.enable_conceal, 2, 5, stream=-1) == ARG    # streams 2, 3, 4 have no strict feed: stream 0 is NOT enabled, stream 1 keeps its own
    assert [b.conceal_cfg(s) for s in range(5)] == [None, (16, 21), None, None, None]
    b.enable_conceal(1, 1, stream=0)
    b.enable_conceal(0, 0, stream=1)                             # hold 0: off (step is not read)
    assert [b.conceal_cfg(s) for s in range(5)] == [(1, 1), None, None, None, None]
    rec = b.conceal_records()
    assert rec.shape == (5,) and not rec.view(np.uint8).any()
    b.enable_conceal(0, stream=-1)                               # off for all is legal whatever the streams' feeds
    assert all(b.conceal_cfg(s) is None for s in range(5))
    b.close()
    a = M.Batch([_scfg(M, 48000, "s", 128)] * 2)                 # every stream a strict feed: -1 goes through
    a.set_feed(-1, fc)
    a.enable_conceal()
    assert [a.conceal_cfg(s) for s in range(2)] == [(4, 3), (4, 3)]
    a.close()


@pytest.mark.gpu
def test_feed_set_and_feed_reset_clear_the_state(M):
    import conceallib as K
    import feedlib as F
    frames = K.case_frames(0)
    fc = M.FeedConfig(**F.feed_cfg_of(K.CASES[0]))
    b = M.Batch([_scfg(M, 48000, "s", 128)] * 3)
    b.set_feed(-1, fc)
    b.enable_conceal(4, 3)
    good = [(frames[0], len(frames[0]))] * 3
    lost = [(b"", 0)] * 3

    def call(slots):
        fr, ln = F.slots_to_arrays([[x] for x in slots], b.feed_stride)
        return b.feed(fr, ln)[0][0]
    call(good)
    pcm = call(lost)
    rec = b.conceal_records()
    assert pcm.any(axis=1).all() and [tuple(int(r[n]) for n in ("frames", "passed", "concealed", "muted", "run", "offset")) for r in rec] == [(2, 1, 1, 0, 1, 3)] * 3
    b.feed_reset(0)                                              # stream 0: G, run and record forgotten, the parameters stay
    b.set_feed(1, fc)                                            # stream 1: a feed set again: concealment off
    assert [b.conceal_cfg(s) for s in range(3)] == [(4, 3), None, (4, 3)]
    rec = b.conceal_records()
    assert not rec[:2].view(np.uint8).any() and int(rec[2]["run"]) == 1
    pcm = call(lost)
    rec = b.conceal_records()
    assert not pcm[0].any() and not pcm[1].any() and pcm[2].any()   # no G; no concealment; the second repeat
    assert (int(rec[0]["muted"]), int(rec[0]["concealed"]), int(rec[0]["run"])) == (1, 0, 1) and not rec[1:2].view(np.uint8).any()
    assert (int(rec[2]["concealed"]), int(rec[2]["run"]), int(rec[2]["offset"])) == (2, 2, 6)
    b.stream_reset(2)                                            # implies tlb_feed_reset
    assert not b.conceal_records()[2:].view(np.uint8).any() and b.conceal_cfg(2) == (4, 3)
    b.set_feed(2, None)                                          # removal
    assert b.conceal_cfg(2) is None
    b.conceal_reset(0)
    assert not b.conceal_records().view(np.uint8).any()
    b.close()
