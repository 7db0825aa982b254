#!/usr/bin/env python3
"""What a record option adds to a tick, and what this commit costs an object with and without it, on the GPU.

    python tools/tick_record_cost.py --option monitor|compare|loudness|lra|truepeak|limiter|all|conceal [--streams 16384] [--psy 3] [--ticks 200] [--rounds 5]
                                     [--hot] [--parent-lib PATH] [--out profiles/tick_records.txt]

The record options of a tick object (csrc/tlb_tick.cpp, tick_records): `monitor` (tlb_tick_enable_monitor, TLB_MONITOR_AUDIO), `compare`
(tlb_tick_enable_compare with the default params; its `off` legs have the AUDIO monitor it needs), `loudness`, `truepeak`, and `all` four; `lra`
(tlb_tick_enable_lra: its `off` legs have the loudness meter it counts in, so that `on - off` is the counting of range blocks alone); and `limiter`
(tlb_tick_enable_limiter, the defaults: it runs AHEAD of the encoder; --hot clips the input 30 dB up, so that its active path runs on every frame -- the encoder then
encodes another signal in every leg, so hot legs compare with hot legs only).
One tick object per leg -- `parent` and `parent-on` (--parent-lib: a libtoolame_dab_hip.so built from the parent commit, loaded beside this
one; `parent-on` only when that library has the option's entry points), `off` (this library, the option never enabled) and `on` -- all
48 kHz stereo 128 kbps, egress EDI AF, the legs interleaved round by round in one process on one box.  Every round runs `ticks` ticks of
tlb_tick_run per leg and keeps the median and the maximum of tlb_tick_last_ms (device clock: first copy-in queued -> last copy-out done,
the records' copy-out included).  The file gets the medians, minima and maxima over the rounds.  The condition: `off` makes the device
calls `parent` makes and `on` those `parent-on` makes, so each median belongs inside its parent leg's own run-to-run spread.  A leg that
cannot be run is written as NOT MEASURED with the reason.
`conceal` (tlb_tick_enable_conceal, hold 4, step 3) is measured on another workload, since it lives on the feed path: every stream on a strict 192 kbps
Layer II feed (no PCM crosses the link).  Legs: `parent` (--parent-lib), `off` (this library, never enabled), and three with concealment on:
`on-0` no slot lost, `on-10` every tenth slot of every stream lost (staggered over the streams), `on-all` every slot lost (every unit
synthesises as long as hold lasts, so the leg's ticks are cut into runs of hold + 1 lost slots and one good one -- but the feed kernel then
decodes next to nothing), and `on-alt` every other slot lost, staggered: every unit of the concealment kernel synthesises (a lost slot, or the
good slot behind one) while the feed kernel still decodes half the slots -- the most work the option can ADD to a tick."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

# option -> (what its `off` legs enable, what its `on` legs enable on top), by the names below
OPTIONS = {"monitor": ((), ("monitor",)), "compare": (("monitor",), ("compare",)), "loudness": ((), ("loudness",)), "lra": (("loudness",), ("lra",)), "truepeak": ((), ("truepeak",)), "limiter": ((), ("limiter",)),
           "all": ((), ("monitor", "compare", "loudness", "truepeak"))}
ENABLE = {"monitor": lambda t: t.enable_monitor("audio"), "compare": lambda t: t.enable_compare(), "loudness": lambda t: t.enable_loudness(), "lra": lambda t: t.enable_lra(),
          "truepeak": lambda t: t.enable_truepeak(), "limiter": lambda t: t.enable_limiter()}
# ... and a count from the option's records, to show that it ran
MEASURED = {"monitor": lambda t: t.monitor["frames"], "compare": lambda t: t.compare["frames_compared"], "loudness": lambda t: t.loudness["frames"], "lra": lambda t: t.lra()["blocks"],
            "truepeak": lambda t: t.truepeak["frames"], "limiter": lambda t: t.limiter["frames"]}


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %.4f  min %.4f  max %.4f  (rounds: %s)" % (np.median(v), v.min(), v.max(), " ".join("%.4f" % x for x in v))


def main_conceal(args):
    import torch
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as TL
    from pcmgen import gen_pcm
    import declib as D
    ns, hold, step = args.streams, 4, 3
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=args.psy)] * ns
    src = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=192, psy_model=1)])      # eight source frames; stream s is fed frame s % 8 every tick
    data, _ = src.encode(gen_pcm(7, 0, 0, 8)[:, None])
    frames = D.cut_frames(data[0] + src.flush()[0], dict(samplerate=48000, kbps=192))
    src.close()
    assert len(frames) == 8 and all(len(f) == 576 for f in frames)
    rows = np.stack([np.frombuffer(frames[s % 8], dtype=np.uint8) for s in range(ns)])
    legs, why = {}, {}                                               # leg -> (library, concealment on, which (tick, stream) slots are lost)
    if args.parent_lib and Path(args.parent_lib).exists():
        legs["parent"] = (TL._bind(C.CDLL(str(Path(args.parent_lib).resolve()))), False, None)
    else:
        why["parent"] = "no library of the parent commit was given (--parent-lib)"
    sidx = np.arange(ns)
    legs["off"] = (None, False, None)
    legs["on-0"] = (None, True, None)
    legs["on-10"] = (None, True, lambda i: (i + sidx) % 10 == 0)
    legs["on-all"] = (None, True, lambda i: np.full(ns, i % (hold + 2) != 0))      # one good slot, then hold + 1 lost ones that all synthesise
    legs["on-alt"] = (None, True, lambda i: (i + sidx) % 2 == 0)
    objs, count = {}, {}
    for name, (lib, on, lost) in legs.items():
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=lib)
        t.set_feed(-1, M.FeedConfig(48000, 192, 2))
        if on:
            t.enable_conceal(hold, step)
        for _ in range(6):                                            # both input sets' frames, and the warm-up: code objects loaded, every buffer touched
            t.feed[:, :576] = rows
            t.feed_len[:] = 576
            t.run()
        objs[name], count[name] = t, 0
    out = {k: {"median_ms": [], "max_ms": []} for k in objs}
    for _ in range(args.rounds):
        for name, t in objs.items():
            lost = legs[name][2]
            dev = np.empty(args.ticks)
            for i in range(args.ticks):
                t.feed_len[:] = 576 if lost is None else np.where(lost(count[name]), 0, 576)
                count[name] += 1
                t.run()
                dev[i] = t.last_ms()
            out[name]["median_ms"].append(float(np.median(dev)))
            out[name]["max_ms"].append(float(dev.max()))
    recs = {n: {f: int(objs[n].conceal()[f].sum()) for f in ("frames", "passed", "concealed", "muted")} for n in objs if legs[n][1]}
    for t in objs.values():
        t.close()
    lines = ["tools/tick_record_cost.py --option conceal on %s: %d streams of 48 kHz stereo 128 kbps psy %d, every stream on a strict 192 kbps feed," %
             (torch.cuda.get_device_name(0), ns, args.psy),
             "EDI AF, %d ticks of tlb_tick_run per round and leg, %d rounds interleaved in one process.  Per leg: the rounds' medians and maxima of" % (args.ticks, args.rounds),
             "tlb_tick_last_ms (device clock).  A 48 kHz frame lasts 24 ms.  Concealment: hold %d, step %d." % (hold, step)]
    for name in ("parent", "off", "on-0", "on-10", "on-all", "on-alt"):
        if name not in out:
            lines.append("%-9s NOT MEASURED: %s" % (name, why[name]))
            continue
        lines.append("%-9s median of a round ms : %s" % (name, fmt(out[name]["median_ms"])))
        lines.append("%-9s maximum of a round ms: %s" % (name, fmt(out[name]["max_ms"])))
    med = lambda n: float(np.median(out[n]["median_ms"]))
    sp = lambda n: max(out[n]["median_ms"]) - min(out[n]["median_ms"])
    if "parent" in out:
        d = med("off") - med("parent")
        lines.append("(a) off - parent: %+.4f ms; the parent leg's own spread over its rounds: %.4f ms -> %s" % (d, sp("parent"), "inside it" if abs(d) <= sp("parent") else "OUTSIDE it"))
    else:
        lines.append("(a) off - parent: NOT MEASURED")
    for tag, leg, what in (("(b)", "on-0", "enabled, no loss: the units that leave early"), ("(c)", "on-10", "every tenth slot lost"), ("(d)", "on-all", "every slot lost but one in %d" % (hold + 2)),
                           ("(e)", "on-alt", "every other slot lost, staggered: every concealment unit synthesises")):
        lines.append("%s %s - off: %+.4f ms per tick for %d streams (%s; spread of the leg %.4f ms, of off %.4f ms; records: %s)" %
                     (tag, leg, med(leg) - med("off"), ns, what, sp(leg), sp("off"), ", ".join("%s %d" % kv for kv in recs[leg].items())))
    lines.append("131 072 streams: NOT MEASURED.")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", choices=list(OPTIONS) + ["conceal"], required=True)
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
    if args.option == "conceal":
        return main_conceal(args)
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
    lines.append("(c) on - off: %+.4f ms per tick for %d streams (in all: %s)" % (med("on") - med("off"), ns, ", ".join("%s %d %s" % (k, v, "range blocks" if k == "lra" else "frames") for k, v in measured.items())))
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
