#!/usr/bin/env python3
"""Cost of the ingest kernels (csrc/toolame_ingest.hip), with short reads and without, against each other and another build, on the GPU.

    python tools/ingest_short_measure.py kernel [--streams 131072] [--rounds 7] [--launches 50] [--legs existing,valid_full,valid_1pct] [--parent-lib PATH]
    python tools/ingest_short_measure.py tick   [--streams 131072] [--rounds 5] [--ticks 100] [--parent-lib PATH]

kernel: device-resident buffers, one frame of every stream per launch, `launches` launches between two device events, the legs interleaved
round by round -- `existing` = tlb_ingest_device (tl_ingest_kernel: the full-slot text of csrc/mp2_ingest.h that tl_ingest_valid_kernel
shares, alone), `valid_full` = tlb_ingest_device_valid with every slot at 1152,
`valid_1pct` = the same with about 1 % of the slots short by 1..115 frames (the range that is stretched).  With --parent-lib the library of
another build (the parent commit's; before the two kernels shared a text its tl_ingest_kernel was a copy of its own in toolame_hip.hip) is loaded
beside this one and runs a leg `parent_existing` in the same rounds.  Run it under
`rocprofv3 --kernel-trace --stats` with ONE leg per process for per-kernel times (the two builds' kernels carry the same names).
tick: the `tick_pipeline` shape of bench.py (tlb_tick_run, pinned PCM -> PCIe -> ingest -> encode -> EDI AF -> PCIe, psy 3) for a tick object
that never enables short reads, one that does (every read full), one with about 1 % of the streams short per tick, and -- with
--parent-lib -- the parent's, interleaved round by round.  Prints one JSON line; per-leg median, min, max over the rounds (the spread)."""
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


def short_valid(rng, n, share=0.01):
    v = np.full(n, 1152, np.int32)
    k = rng.random(n) < share
    v[k] = 1152 - rng.integers(1, 116, size=int(k.sum()))
    return v


def kernel(args, M, libs):
    import torch
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=3)] * ns
    rng = np.random.default_rng(1)
    d_in = torch.from_numpy(rng.integers(-20000, 20000, size=(ns, 2304), dtype=np.int64).astype(np.int16)).cuda()
    d_pcm = torch.empty((ns, 2, 1152), dtype=torch.int16, device="cuda")
    d_pk = torch.empty((ns, 2), dtype=torch.int16, device="cuda")
    v1 = short_valid(rng, ns)
    d_full = torch.full((ns,), 1152, dtype=torch.int32, device="cuda")
    d_1pct = torch.from_numpy(v1).cuda()
    batches = {name: M.Batch(cfg, lib=L) for name, L in libs.items()}
    legs = {}
    for leg in args.legs.split(","):
        if leg == "existing":
            legs[leg] = lambda b=batches["this"]: b.ingest_device(d_in.data_ptr(), 1, d_pcm.data_ptr(), d_pk.data_ptr())
        elif leg == "parent_existing":
            legs[leg] = lambda b=batches["parent"]: b.ingest_device(d_in.data_ptr(), 1, d_pcm.data_ptr(), d_pk.data_ptr())
        else:
            dv = d_full if leg == "valid_full" else d_1pct
            legs[leg] = lambda b=batches["this"], dv=dv: b.L.tlb_ingest_device_valid(b.h, d_in.data_ptr(), dv.data_ptr(), 1, d_pcm.data_ptr(), d_pk.data_ptr(), None)
    out = {k: [] for k in legs}
    for fn in legs.values():                                          # warm-up: code objects loaded, every buffer touched
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / args.launches * 1e3)       # microseconds per launch
    res = {"what": f"ingest kernels, {ns} streams x 1 frame per launch, {args.launches} launches per timing, us per launch (device events)",
           "short_slots": int((v1 < 1152).sum()), "bytes_moved_per_launch": ns * 2304 * 2 * 2,
           "legs": {k: stats(v) for k, v in out.items()}}
    for b in batches.values():
        b.close()
    return res


def tick(args, M, libs):
    from pcmgen import gen_pcm
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=3)] * ns
    nd = min(ns, 1024)
    base = np.stack([gen_pcm(s, 0, 0, 1)[0].T.reshape(-1) for s in range(nd)])
    rng = np.random.default_rng(2)
    objs = {}
    for name in (["parent_plain"] if "parent" in libs else []) + ["plain", "enabled_full", "enabled_1pct"]:
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=libs["parent" if name == "parent_plain" else "this"])
        if name.startswith("enabled"):
            t.enable_short_reads()
        for _ in range(2):                                            # both input sets
            pcm = t.pcm
            for k in range(0, ns, nd):
                pcm[k:k + nd] = base[:min(nd, ns - k)]
            t.run()
        for _ in range(4):
            t.run()
        objs[name] = t
    out = {k: {"run_ms": [], "device_ms": []} for k in objs}
    for _ in range(args.rounds):
        for name, t in objs.items():
            lat, dev = np.empty(args.ticks), np.empty(args.ticks)
            for i in range(args.ticks):
                if name == "enabled_1pct":
                    t.valid[:] = short_valid(rng, ns)
                a = time.perf_counter()
                t.run()
                lat[i] = time.perf_counter() - a
                dev[i] = t.last_ms()
            out[name]["run_ms"].append(float(np.median(lat)) * 1e3)
            out[name]["device_ms"].append(float(np.median(dev)))
    res = {"what": f"tlb_tick_run, {ns} streams (48 kHz stereo 128 kbps psy 3, EDI AF), {args.ticks} ticks per timing: median host ms per tick and median device ms per tick of each round",
           "legs": {k: {m: stats(v) for m, v in d.items()} for k, d in out.items()}}
    res["underruns_seen"] = int(objs["enabled_1pct"].underruns.sum())
    for t in objs.values():
        t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "tick"])
    ap.add_argument("--streams", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--legs", default="")
    ap.add_argument("--parent-lib", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as T
    libs = {"this": M.load_library()}
    if args.parent_lib:
        libs["parent"] = T._bind(C.CDLL(str(Path(args.parent_lib).resolve())))
    if not args.legs:
        args.legs = ("parent_existing," if args.parent_lib else "") + "existing,valid_full,valid_1pct"
    res = kernel(args, M, libs) if args.mode == "kernel" else tick(args, M, libs)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
