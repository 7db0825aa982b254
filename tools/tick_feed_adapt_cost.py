#!/usr/bin/env python3
"""What ADAPTED Layer II feeds cost and save in a tick (tlb_tick_set_feed_adapted), on the GPU.

    python tools/tick_feed_adapt_cost.py [--streams 16384] [--ticks 100] [--rounds 5] [--psy 3] [--parent-lib PATH] [--check-ticks 4] [--out profiles/tick_feed_adapt.txt]

Tick objects of 48 kHz stereo 128 kbps, egress EDI AF:
    (a) `pcm`      PCM in, no feed set
    (b) `feed`     every stream with a strict 192 kbps feed, no PCM over the link
    (c) `adapted`  every stream with a 44.1 kHz 128 kbps two-channel ADAPTED feed (a frame on the ticks that want one), no PCM over the link
    (d) `source`   the same rate as PCM: set_source(44100), 1058 / 1059 source frames per slot
    `parent_pcm`, `parent_feed`, `parent_adapted`: (a), (b) and (c) with the library built from the PARENT commit (--parent-lib: its
    libtoolame_dab_hip.so; left out without it).  They queue the device calls the parent queues: each must lie within the spread the
    parent's legs show, and after the warm-up round `feed` / `parent_feed` and `adapted` / `parent_adapted` are stepped --check-ticks ticks
    side by side and must deliver byte-identical AF packets for every stream (asserted).
The legs are interleaved round by round in one process on one box.  A round runs `ticks` ticks per leg overlapped as an application does
(submit, submit, wait, submit, wait, ...) and keeps the median FINISHED-TICK INTERVAL (wall clock between two waits returning) and the
median and maximum of tlb_tick_last_ms (device clock: first copy-in queued -> last copy-out done).  The input sets are filled once; a
tick refreshes only the feed lengths (a set comes back all 0; the adapted leg leaves them 0 on the ticks that want no frame).  Bytes over
the host-to-device link per tick are what the submit copies in: 4608 per stream for PCM (with a source rate 4232 / 4236 of them are read),
the feed's slot + 4 per stream for a feed.  Prints one JSON line, and writes it with a readable table to --out; no pass / fail: (c)
against (d) is reported, with which of the two finishes ticks faster at this size."""
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
    ap.add_argument("--psy", type=int, default=3)
    ap.add_argument("--check-ticks", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as T
    from pcmgen import gen_pcm
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=args.psy)] * ns
    fc = M.FeedConfig(48000, 192, 2)
    fa = M.FeedConfig(44100, 128, 2)
    nd = min(ns, 1024)
    pcm = gen_pcm(1, 0, 0, 2)
    base = np.stack([gen_pcm(s, 0, 0, 1)[0].T.reshape(-1) for s in range(nd)])
    src = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=192, psy_model=1)])      # two 192 kbps frames of audio: the feed
    data, _ = src.encode(pcm[:, None])
    frames = [data[0][:576], src.flush()[0]]
    src.close()
    assert all(len(f) == 576 for f in frames)
    src = M.Batch([M.StreamConfig(samplerate=44100, mode="s", bitrate=128, psy_model=1)])       # two 44.1 kHz 128 kbps frames: the adapted feed
    data, _ = src.encode(pcm[:, None])
    aframes = [data[0], src.flush()[0]]
    src.close()
    assert all(len(f) in (417, 418) for f in aframes)
    plib = T._bind(C.CDLL(str(args.parent_lib))) if args.parent_lib else None
    legs = ["pcm", "feed", "adapted", "source"] + (["parent_pcm", "parent_feed", "parent_adapted"] if plib else [])
    fed = {"feed": (fc, frames), "parent_feed": (fc, frames), "adapted": (fa, aframes), "parent_adapted": (fa, aframes)}
    objs, link = {}, {}
    for name in legs:
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=plib if name.startswith("parent") else None)
        if name.endswith("adapted"):
            t.set_feed(-1, fa, adapt=True)
        elif name in fed:
            t.set_feed(-1, fc)
        if name == "source":
            t.set_source(44100)
        link[name] = ns * (t.feed_stride + 4) if name in fed else ns * 4608
        for k in range(2):                                            # both input sets, once
            if name in fed:
                b = fed[name][1][k]
                t.feed[:, :len(b)] = np.frombuffer(b, dtype=np.uint8)
                t.feed_len[:] = len(b)
            else:
                p = t.pcm
                for i in range(0, ns, nd):
                    p[i:i + nd] = base[:min(nd, ns - i)]
            t.run()
        if name in fed:
            assert not (t.feed_report["status"] != 0).any()
        objs[name] = t
    out = {k: {"interval_ms": [], "median_ms": [], "max_ms": []} for k in objs}

    nsub = {k: 0 for k in objs}

    def submit(name, t):
        nsub[name] += 1
        if name.endswith("adapted"):                                 # every stream has the one schedule: stream 0 answers for all
            if t.feed_want(0):
                t.feed_len[:] = len(aframes[(nsub[name] - 1) & 1])   # (the two input sets take turns; each holds one of the two frames)
        elif name in fed:
            t.feed_len[:] = 576
        t.submit()

    def same_packets(a, b):
        """both legs have run the same ticks so far: the next ones side by side, every stream's AF packets compared"""
        for i in range(args.check_ticks):
            for name in (a, b):
                submit(name, objs[name])
            for name in (a, b):
                objs[name].wait()
            for s in range(ns):
                pa = objs[a].packets(s)
                assert pa and pa == objs[b].packets(s), f"{a} / {b}: tick {i} of the check, stream {s}: the AF packets differ"
    for rnd in range(args.rounds + 1):                               # round 0 is the warm-up: code objects loaded, every buffer touched
        if rnd == 1 and plib:
            same_packets("feed", "parent_feed")
            same_packets("adapted", "parent_adapted")
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
    res = {"what": f"{ns} streams (48 kHz stereo 128 kbps psy {args.psy}, EDI AF), {args.ticks} overlapped ticks per round and leg, {args.rounds} rounds interleaved; "
                   "interval_ms = wall clock between finished ticks, median_ms / max_ms = tlb_tick_last_ms",
           "legs": {k: {m: stats(v) for m, v in d.items()} for k, d in out.items()},
           "same_af_packets": {"ticks": args.check_ticks, "pairs": ["feed/parent_feed", "adapted/parent_adapted"]} if plib else None,
           "link_bytes_per_tick": link, "link_bytes_per_stream": {k: v // ns for k, v in link.items()}}
    for t in objs.values():
        t.close()
    res["device"] = torch.cuda.get_device_name(0)
    iv = {k: res["legs"][k]["interval_ms"]["median"] for k in res["legs"]}
    res["adapted_vs_source"] = {"adapted_ms": iv["adapted"], "source_ms": iv["source"], "faster": "adapted" if iv["adapted"] < iv["source"] else "source"}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write(f"# {res['what']}; {res['device']}\n")
            for k, d in res["legs"].items():
                f.write(f"{k:12s} interval {d['interval_ms']['median']:9.4f} ms (rounds {d['interval_ms']['min']:.4f} .. {d['interval_ms']['max']:.4f})  "
                        f"tlb_tick_last_ms {d['median_ms']['median']:9.4f}  link {res['link_bytes_per_stream'][k]} bytes per stream and tick\n")
            f.write(f"(c) against (d): the {res['adapted_vs_source']['faster']} leg finishes ticks faster at this size\n")
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
