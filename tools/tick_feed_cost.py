#!/usr/bin/env python3
"""What Layer II feeds cost and save in a tick (tlb_tick_set_feed), on the GPU.

    python tools/tick_feed_cost.py [--streams 16384] [--ticks 100] [--rounds 5] [--parent-lib PATH]

Tick objects of 48 kHz stereo 128 kbps psy 1, egress EDI AF:
    (a) `pcm`     PCM in, this commit's library, no feed set
    (b) `parent`  PCM in, the library built from the PARENT commit (--parent-lib: its libtoolame_dab_hip.so; the leg is left out without it)
    (c) `feed`    every stream fed at 192 kbps, no PCM over the link
The legs are interleaved round by round in one process on one box.  A round runs `ticks` ticks per leg overlapped as an application does
(submit, submit, wait, submit, wait, ...) and keeps the median FINISHED-TICK INTERVAL (wall clock between two waits returning) and the
median and maximum of tlb_tick_last_ms (device clock: first copy-in queued -> last copy-out done).  The input sets are filled once; a
tick refreshes only the feed lengths (a set comes back all 0).  Bytes over the host-to-device link per tick are what the submit copies in:
4608 per stream for PCM, the feed's slot + 4 per stream for a feed.  Prints one JSON line; no pass / fail."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "rounds": [round(float(x), 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as T
    from pcmgen import gen_pcm
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1)] * ns
    fc = M.FeedConfig(48000, 192, 2)
    nd = min(ns, 1024)
    pcm = gen_pcm(1, 0, 0, 2)
    base = np.stack([gen_pcm(s, 0, 0, 1)[0].T.reshape(-1) for s in range(nd)])
    src = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=192, psy_model=1)])      # two 192 kbps frames of audio: the feed
    data, _ = src.encode(pcm[:, None])
    frames = [data[0][:576], src.flush()[0]]
    src.close()
    assert all(len(f) == 576 for f in frames)
    legs = ["pcm", "feed"] + (["parent"] if args.parent_lib else [])
    objs, link = {}, {}
    for name in legs:
        lib = T._bind(C.CDLL(str(args.parent_lib))) if name == "parent" else None
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=lib)
        if name == "feed":
            t.set_feed(-1, fc)
        link[name] = ns * (t.feed_stride + 4) if name == "feed" else ns * 4608
        for k in range(2):                                            # both input sets, once
            if name == "feed":
                t.feed[:, :576] = np.frombuffer(frames[k], dtype=np.uint8)
                t.feed_len[:] = 576
            else:
                p = t.pcm
                for i in range(0, ns, nd):
                    p[i:i + nd] = base[:min(nd, ns - i)]
            t.run()
        if name == "feed":
            assert not (t.feed_report["status"] != 0).any()
        objs[name] = t
    out = {k: {"interval_ms": [], "median_ms": [], "max_ms": []} for k in objs}

    def submit(name, t):
        if name == "feed":
            t.feed_len[:] = 576
        t.submit()
    for rnd in range(args.rounds + 1):                               # round 0 is the warm-up: code objects loaded, every buffer touched
        for name, t in objs.items():
            dev, done = np.empty(args.ticks), np.empty(args.ticks)
            submit(name, t)
            for i in range(args.ticks):
                if i + 1 < args.ticks:
                    submit(name, t)
                t.wait()
                done[i] = time.perf_counter()
                dev[i] = t.last_ms()
            if rnd:
                out[name]["interval_ms"].append(float(np.median(np.diff(done))) * 1e3)
                out[name]["median_ms"].append(float(np.median(dev)))
                out[name]["max_ms"].append(float(dev.max()))
    res = {"what": f"{ns} streams (48 kHz stereo 128 kbps psy 1, EDI AF), {args.ticks} overlapped ticks per round and leg, {args.rounds} rounds interleaved; "
                   "interval_ms = wall clock between finished ticks, median_ms / max_ms = tlb_tick_last_ms",
           "legs": {k: {m: stats(v) for m, v in d.items()} for k, d in out.items()},
           "link_bytes_per_tick": link, "link_bytes_per_stream": {k: v // ns for k, v in link.items()}}
    for t in objs.values():
        t.close()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
