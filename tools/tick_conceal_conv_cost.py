#!/usr/bin/env python3
"""What the feed concealment costs a tick on ADAPTED and DOWN feeds (tlb_tick_enable_feed_loss; csrc/toolame_conceal_conv.hip) -- the sibling
of `tools/tick_record_cost.py --option conceal`, which measures it on strict feeds.

    python tools/tick_conceal_conv_cost.py [--streams 16384] [--psy 3] [--ticks 200] [--rounds 5] [--parent-lib PATH]
                                           [--out profiles/tick_conceal_conv.txt]

Two workloads, one after the other: every stream a 48 kHz stereo 128 kbps service on a 44.1 kHz 128 kbps ADAPTED feed, and every stream a
24 kHz stereo 64 kbps service on a 48 kHz 192 kbps DOWN feed (no PCM crosses the link in either).  Per workload one tick object per leg:
`parent` (--parent-lib: a libtoolame_dab_hip.so built from the parent commit, loaded beside this one, concealment never enabled), `off`
(this library, never enabled), `on-0` (enabled, hold 4, step 3, nothing lost), `on-10` (every tenth WANTED slot lost, staggered over the
streams) and `on-alt` (every other wanted slot lost, staggered: every unit of the conceal kernel synthesises, a lost slot or the good one
behind it).  The legs run interleaved, round after round, in one process; per leg the rounds' medians of tlb_tick_last_ms (device clock).
The first round of every leg is slow on a fresh device (clocks, first touches): one round more than --rounds is run and the first is thrown away.
The one bound: `off` queues the kernels `parent` queues, so its median belongs inside the parent leg's own run-to-run spread."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HOLD, STEP = 4, 3
WORKLOADS = {"adapted": dict(feed=(44100, 128), enc=(48000, 128)), "down": dict(feed=(48000, 192), enc=(24000, 64))}


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %.4f  min %.4f  max %.4f  (rounds: %s)" % (np.median(v), v.min(), v.max(), " ".join("%.4f" % x for x in v))


def measure(args, kind):
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as TL
    from pcmgen import gen_pcm
    import declib as D
    ns = args.streams
    (frate, fkbps), (erate, ekbps) = WORKLOADS[kind]["feed"], WORKLOADS[kind]["enc"]
    cfg = [M.StreamConfig(samplerate=erate, mode="s", bitrate=ekbps, psy_model=args.psy)] * ns
    src = M.Batch([M.StreamConfig(samplerate=frate, mode="s", bitrate=fkbps, psy_model=1)])      # eight source frames; stream s is fed frame s % 8 in every wanted slot
    data, _ = src.encode(gen_pcm(7, 0, 0, 8)[:, None])
    frames = D.cut_frames(data[0] + src.flush()[0], dict(samplerate=frate, kbps=fkbps))
    src.close()
    assert len(frames) == 8
    width = max(len(f) for f in frames)
    rows = np.zeros((ns, width), dtype=np.uint8)
    lens = np.zeros(ns, dtype=np.int32)
    for s in range(ns):
        f = frames[s % 8]
        rows[s, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        lens[s] = len(f)
    sidx = np.arange(ns)
    legs, why = {}, {}                                               # leg -> (library, concealment on, which streams lose wanted slot k)
    if args.parent_lib and Path(args.parent_lib).exists():
        legs["parent"] = (TL._bind(C.CDLL(str(Path(args.parent_lib).resolve()))), False, None)
    else:
        why["parent"] = "no library of the parent commit was given (--parent-lib)"
    legs["off"] = (None, False, None)
    legs["on-0"] = (None, True, None)
    legs["on-10"] = (None, True, lambda k: (k + sidx) % 10 == 0)
    legs["on-alt"] = (None, True, lambda k: (k + sidx) % 2 == 0)
    fc = M.FeedConfig(frate, fkbps, 2)

    def tick(t, lost, k):
        """one tick: every wanted slot filled but the lost ones -> the wanted slots so far"""
        if kind == "down":
            for j in range(t.down_feed_want(0)):                     # (every stream has the one configuration: all want the same)
                t.down_feed[:, j, :width] = rows
                t.down_feed_len[:, j] = lens if lost is None else np.where(lost(k), 0, lens)
                k += 1
        elif t.feed_want(0):
            t.feed[:, :width] = rows
            t.feed_len[:] = lens if lost is None else np.where(lost(k), 0, lens)
            k += 1
        t.run()
        return k

    objs, count = {}, {}
    for name, (lib, on, lost) in legs.items():
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=lib)
        if kind == "down":
            t.set_down_feed(-1, fc)
        else:
            t.set_feed(-1, fc, adapt=True)
        if on:
            t.enable_conceal(HOLD, STEP, any_feed=True)
        k = 0
        for _ in range(6):                                            # the warm-up: code objects loaded, every buffer touched
            k = tick(t, None, k)
        objs[name], count[name] = t, k
    out = {k: {"median_ms": [], "max_ms": []} for k in objs}
    for rnd in range(args.rounds + 1):                                # round 0 is the warm-up round: run like the others, not recorded
        for name, t in objs.items():
            dev = np.empty(args.ticks)
            for i in range(args.ticks):
                count[name] = tick(t, legs[name][2], count[name])
                dev[i] = t.last_ms()
            if rnd == 0:
                continue
            out[name]["median_ms"].append(float(np.median(dev)))
            out[name]["max_ms"].append(float(dev.max()))
    recs = {n: {f: int(objs[n].conceal()[f].sum()) for f in ("frames", "passed", "concealed", "muted")} for n in objs if legs[n][1]}
    for t in objs.values():
        t.close()
    lines = ["%s feeds: %d streams of %d Hz stereo %d kbps psy %d, every stream on a %d Hz %d kbps %s feed, EDI AF, %d ticks of tlb_tick_run per round and leg," %
             (kind.upper(), ns, erate, ekbps, args.psy, frate, fkbps, kind, args.ticks),
             "%d rounds interleaved in one process behind one unrecorded warm-up round of the same length.  Per leg: the rounds' medians and maxima of tlb_tick_last_ms (device clock).  A frame lasts %d ms." % (args.rounds, 1152000 // erate),
             "Concealment: hold %d, step %d." % (HOLD, STEP)]
    for name in ("parent", "off", "on-0", "on-10", "on-alt"):
        if name not in out:
            lines.append("%-9s NOT MEASURED: %s" % (name, why[name]))
            continue
        lines.append("%-9s median of a round ms : %s" % (name, fmt(out[name]["median_ms"])))
        lines.append("%-9s maximum of a round ms: %s" % (name, fmt(out[name]["max_ms"])))
    med = lambda n: float(np.median(out[n]["median_ms"]))
    sp = lambda n: max(out[n]["median_ms"]) - min(out[n]["median_ms"])
    if "parent" in out:
        d = med("off") - med("parent")
        lines.append("(1) never enabled, off - parent: %+.4f ms; the parent leg's own spread over its rounds: %.4f ms -> %s" % (d, sp("parent"), "inside it" if abs(d) <= sp("parent") else "OUTSIDE it"))
    else:
        lines.append("(1) never enabled, off - parent: NOT MEASURED")
    for tag, leg, what in (("(2)", "on-0", "enabled, nothing lost: the units that leave early"), ("(3)", "on-10", "every tenth wanted slot lost"),
                           ("(4)", "on-alt", "every other wanted slot lost, staggered: every conceal unit of a wanted slot synthesises")):
        lines.append("%s %s - off: %+.4f ms per tick for %d streams (%s; spread of the leg %.4f ms, of off %.4f ms; records: %s)" %
                     (tag, leg, med(leg) - med("off"), ns, what, sp(leg), sp("off"), ", ".join("%s %d" % kv for kv in recs[leg].items())))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--psy", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tick_conceal_conv.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    lines = ["tools/tick_conceal_conv_cost.py on %s" % torch.cuda.get_device_name(0)]
    for kind in WORKLOADS:
        lines += [""] + measure(args, kind)
    lines += ["", "131 072 streams: NOT MEASURED."]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
