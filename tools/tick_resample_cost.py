#!/usr/bin/env python3
"""What the device resampler adds to a tick (tlb_tick_set_source), on the GPU.

    python tools/tick_resample_cost.py [--streams 16384] [--ticks 200] [--rounds 5]

Two tick objects, 48 kHz stereo 128 kbps psy 1, egress EDI AF: leg `plain` is fed 48 kHz PCM and sets no source, leg `resample` has every
stream at 44.1 kHz (tlb_tick_need frames per slot).  The legs are interleaved round by round in one process on one box; every round runs
`ticks` ticks of tlb_tick_run per leg and keeps the median and the maximum of tlb_tick_last_ms (device clock: first copy-in queued -> last
copy-out done).  Prints one JSON line: per leg the median, min and max over the rounds of both figures, the difference of the medians, and
whether the worst `resample` tick stayed inside the 24 ms a 48 kHz frame lasts."""
import argparse
import json
import sys
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
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from pcmgen import gen_pcm
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1)] * ns
    nd = min(ns, 1024)
    base = np.stack([gen_pcm(s, 0, 0, 1)[0].T.reshape(-1) for s in range(nd)])      # a slot's first 1058 / 1059 frames serve as 44.1 kHz source
    objs = {}
    for name in ("plain", "resample"):
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench")
        if name == "resample":
            t.set_source(44100)
        for _ in range(2):                                            # both input sets
            pcm = t.pcm
            for k in range(0, ns, nd):
                pcm[k:k + nd] = base[:min(nd, ns - k)]
            t.run()
        for _ in range(4):                                            # warm-up: code objects loaded, every buffer touched
            t.run()
        objs[name] = t
    out = {k: {"median_ms": [], "max_ms": []} for k in objs}
    for _ in range(args.rounds):
        for name, t in objs.items():
            dev = np.empty(args.ticks)
            for i in range(args.ticks):
                t.run()
                dev[i] = t.last_ms()
            out[name]["median_ms"].append(float(np.median(dev)))
            out[name]["max_ms"].append(float(dev.max()))
    res = {"what": f"tlb_tick_last_ms of tlb_tick_run, {ns} streams (48 kHz stereo 128 kbps psy 1, EDI AF), {args.ticks} ticks per round and leg, {args.rounds} rounds interleaved",
           "legs": {k: {m: stats(v) for m, v in d.items()} for k, d in out.items()}}
    res["resample_minus_plain_median_ms"] = round(float(np.median(out["resample"]["median_ms"]) - np.median(out["plain"]["median_ms"])), 4)
    res["resample_worst_tick_ms"] = max(out["resample"]["max_ms"])
    res["resample_inside_24_ms"] = bool(res["resample_worst_tick_ms"] < 24.0)
    for t in objs.values():
        t.close()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
