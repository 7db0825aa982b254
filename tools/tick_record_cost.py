#!/usr/bin/env python3
"""What a record option adds to a tick, and what this commit costs an object with and without it, on the GPU.

    python tools/tick_record_cost.py --option monitor|compare|loudness|truepeak|limiter|all [--streams 16384] [--psy 3] [--ticks 200] [--rounds 5]
                                     [--hot] [--parent-lib PATH] [--out profiles/tick_records.txt]

The record options of a tick object (csrc/tlb_tick.cpp, tick_records): `monitor` (tlb_tick_enable_monitor, TLB_MONITOR_AUDIO), `compare`
(tlb_tick_enable_compare with the default params; its `off` legs have the AUDIO monitor it needs), `loudness`, `truepeak`, and `all` four; and `limiter`
(tlb_tick_enable_limiter, the defaults: it runs AHEAD of the encoder; --hot clips the input 30 dB up, so that its active path runs on every frame -- the encoder then
encodes another signal in every leg, so hot legs compare with hot legs only).
One tick object per leg -- `parent` and `parent-on` (--parent-lib: a libtoolame_dab_hip.so built from the parent commit, loaded beside this
one; `parent-on` only when that library has the option's entry points), `off` (this library, the option never enabled) and `on` -- all
48 kHz stereo 128 kbps, egress EDI AF, the legs interleaved round by round in one process on one box.  Every round runs `ticks` ticks of
tlb_tick_run per leg and keeps the median and the maximum of tlb_tick_last_ms (device clock: first copy-in queued -> last copy-out done,
the records' copy-out included).  The file gets the medians, minima and maxima over the rounds.  The condition: `off` makes the device
calls `parent` makes and `on` those `parent-on` makes, so each median belongs inside its parent leg's own run-to-run spread.  A leg that
cannot be run is written as NOT MEASURED with the reason."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

# option -> (what its `off` legs enable, what its `on` legs enable on top), by the names below
OPTIONS = {"monitor": ((), ("monitor",)), "compare": (("monitor",), ("compare",)), "loudness": ((), ("loudness",)), "truepeak": ((), ("truepeak",)), "limiter": ((), ("limiter",)),
           "all": ((), ("monitor", "compare", "loudness", "truepeak"))}
ENABLE = {"monitor": lambda t: t.enable_monitor("audio"), "compare": lambda t: t.enable_compare(), "loudness": lambda t: t.enable_loudness(),
          "truepeak": lambda t: t.enable_truepeak(), "limiter": lambda t: t.enable_limiter()}
# ... and a count from the option's records, to show that it ran
MEASURED = {"monitor": lambda t: t.monitor["frames"], "compare": lambda t: t.compare["frames_compared"], "loudness": lambda t: t.loudness["frames"],
            "truepeak": lambda t: t.truepeak["frames"], "limiter": lambda t: t.limiter["frames"]}


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %.4f  min %.4f  max %.4f  (rounds: %s)" % (np.median(v), v.min(), v.max(), " ".join("%.4f" % x for x in v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", choices=list(OPTIONS), required=True)
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--psy", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hot", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tick_records.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as TL
    from pcmgen import gen_pcm
    ns = args.streams
    base, extra = OPTIONS[args.option]
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=args.psy)] * ns
    nd = min(ns, 1024)
    pcm0 = np.stack([gen_pcm(s, 0, 0, 1)[0].T.reshape(-1) for s in range(nd)])
    if args.hot:
        pcm0 = np.clip(pcm0.astype(np.int64) * 32, -32768, 32767).astype(np.int16)
    legs, why = {}, {}                                               # leg -> (library, what it enables)
    if args.parent_lib and Path(args.parent_lib).exists():
        parent = TL._bind(C.CDLL(str(Path(args.parent_lib).resolve())))
        legs["parent"] = (parent, base)
        missing = [o for o in base + extra if not hasattr(parent, "tlb_tick_enable_" + o)]
        if missing:
            why["parent-on"] = "the parent library has no tlb_tick_enable_" + missing[0]
        else:
            legs["parent-on"] = (parent, base + extra)
    else:
        why["parent"] = why["parent-on"] = "no library of the parent commit was given (--parent-lib)"
    legs["off"] = (None, base)
    legs["on"] = (None, base + extra)
    objs = {}
    for name, (lib, enables) in legs.items():
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=lib)
        for o in enables:
            ENABLE[o](t)
        for _ in range(2):                                            # both input sets
            pcm = t.pcm
            for k in range(0, ns, nd):
                pcm[k:k + nd] = pcm0[:min(nd, ns - k)]
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
    measured = {o: int(MEASURED[o](objs["on"]).sum()) for o in extra}
    if "limiter" in extra:
        measured["limiter: limited"] = int(objs["on"].limiter["limited"].sum())
    for t in objs.values():
        t.close()
    lines = ["tools/tick_record_cost.py --option %s on %s: %d streams of 48 kHz stereo 128 kbps psy %d, EDI AF, %d ticks of tlb_tick_run per round" %
             (args.option + (" --hot" if args.hot else ""), torch.cuda.get_device_name(0), ns, args.psy, args.ticks),
             "and leg, %d rounds interleaved in one process.  Per leg: the rounds' medians and maxima of tlb_tick_last_ms (device clock).  A 48 kHz frame" % args.rounds,
             "lasts 24 ms.  The `off` legs enable: %s; the `on` legs on top of it: %s." % (", ".join(base) or "nothing", ", ".join(extra))]
    for name in ("parent", "parent-on", "off", "on"):
        if name not in out:
            lines.append("%-9s NOT MEASURED: %s" % (name, why[name]))
            continue
        lines.append("%-9s median of a round ms : %s" % (name, fmt(out[name]["median_ms"])))
        lines.append("%-9s maximum of a round ms: %s" % (name, fmt(out[name]["max_ms"])))
    med = lambda n: float(np.median(out[n]["median_ms"]))
    for tag, leg, ref in (("(a)", "off", "parent"), ("(b)", "on", "parent-on")):
        if ref not in out:
            lines.append("%s %s - %s: NOT MEASURED" % (tag, leg, ref))
            continue
        spread = max(out[ref]["median_ms"]) - min(out[ref]["median_ms"])
        d = med(leg) - med(ref)
        lines.append("%s %s - %s: %+.4f ms; the %s leg's own spread over its rounds: %.4f ms -> %s" % (tag, leg, ref, d, ref, spread, "inside it" if abs(d) <= spread else "OUTSIDE it"))
    lines.append("(c) on - off: %+.4f ms per tick for %d streams (in all: %s)" % (med("on") - med("off"), ns, ", ".join("%s %d frames" % kv for kv in measured.items())))
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
