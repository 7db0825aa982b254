#!/usr/bin/env python3
"""What the true-peak meter adds to a tick (tlb_tick_enable_truepeak), and what this commit costs an object that never enables it, on the GPU.

    python tools/tick_truepeak_cost.py [--streams 16384] [--ticks 200] [--rounds 5] [--parent-lib PATH] [--out profiles/tick_truepeak.txt]

One tick object per leg -- `parent` (--parent-lib: a libtoolame_dab_hip.so built from the parent commit, loaded beside this one), `off` (this
library, never enabled) and `on` (tlb_tick_enable_truepeak) -- all 48 kHz stereo 128 kbps psy 3, egress EDI AF, the legs interleaved round
by round in one process on one box.  Every round runs `ticks` ticks of tlb_tick_run per leg and keeps the median and the maximum of
tlb_tick_last_ms (device clock: first copy-in queued -> last copy-out done, the records' copy-out included).  The file gets the medians,
minima and maxima over the rounds.  The condition: `off` makes the device calls the parent makes, so its median belongs inside the parent
leg's own run-to-run spread.  `on` reads the tick's planar PCM once more: 4608 bytes per stereo stream and tick, printed with the bandwidth
the difference to `off` would imply if that read were all of it.  A leg that cannot be run is written as NOT MEASURED with the reason."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %.4f  min %.4f  max %.4f  (rounds: %s)" % (np.median(v), v.min(), v.max(), " ".join("%.4f" % x for x in v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tick_truepeak.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as TL
    from pcmgen import gen_pcm
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=3)] * ns
    nd = min(ns, 1024)
    base = np.stack([gen_pcm(s, 0, 0, 1)[0].T.reshape(-1) for s in range(nd)])
    libs, why = {"off": None, "on": None}, {}
    if args.parent_lib and Path(args.parent_lib).exists():
        libs = {"parent": TL._bind(C.CDLL(str(Path(args.parent_lib).resolve()))), **libs}
    else:
        why["parent"] = "no library of the parent commit was given (--parent-lib)"
    objs = {}
    for name, lib in libs.items():
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=lib)
        if name == "on":
            t.enable_truepeak()
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
    measured = int(objs["on"].truepeak["frames"].sum())
    for t in objs.values():
        t.close()
    lines = ["tools/tick_truepeak_cost.py on %s: %d streams of 48 kHz stereo 128 kbps psy 3, EDI AF, %d ticks of tlb_tick_run per round and leg," % (torch.cuda.get_device_name(0), ns, args.ticks),
             "%d rounds interleaved in one process.  Per leg: the rounds' medians and maxima of tlb_tick_last_ms (device clock).  A 48 kHz frame lasts 24 ms." % args.rounds]
    for name in ("parent", "off", "on"):
        if name not in out:
            lines.append("%-7s NOT MEASURED: %s" % (name, why[name]))
            continue
        lines.append("%-7s median of a round ms : %s" % (name, fmt(out[name]["median_ms"])))
        lines.append("%-7s maximum of a round ms: %s" % (name, fmt(out[name]["max_ms"])))
    med = lambda n: float(np.median(out[n]["median_ms"]))
    if "parent" in out:
        spread = max(out["parent"]["median_ms"]) - min(out["parent"]["median_ms"])
        d = med("off") - med("parent")
        lines.append("(a) off - parent: %+.4f ms; the parent's own spread over its rounds: %.4f ms -> %s" % (d, spread, "inside it" if abs(d) <= spread else "OUTSIDE it"))
    else:
        lines.append("(a) off - parent: NOT MEASURED")
    d = med("on") - med("off")
    lines.append("(b) on - off    : %+.4f ms per tick for %d streams (%d frames measured in all)" % (d, ns, measured))
    pcm_bytes = ns * 2 * 1152 * 2
    lines.append("    the meter reads %d bytes of PCM per tick (%.1f MB) and does %d multiply-adds (%.2f G); the read alone in %.4f ms would be %s" %
                 (pcm_bytes, pcm_bytes / 1e6, ns * 2 * 1152 * 36, ns * 2 * 1152 * 36 / 1e9, d, "%.0f GB/s" % (pcm_bytes / (d * 1e-3) / 1e9) if d > 0 else "unbounded (no cost seen)"))
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
