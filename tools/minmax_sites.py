#!/usr/bin/env python3
"""tools/minmax_sites.py listing.s [mangled kernel name] -- static count, in one kernel of a gfx950 listing (`make -C odr-audioenc_amd/csrc asm`),
of the places where one v_max_f64 / v_min_f64 could stand (csrc/tl_libm.h: tlm_max_gt and its kin):
  * an fp64 compare (gt, lt, ge, le, ngt, nlt, nge, nle) of two register pairs whose mask, until it is overwritten, feeds v_cndmask_b32 only,
    at least two of them, each choosing between a half of one compared value and a half of the other (a high half made by
    v_and_b32 0x7fffffff just before counts as the value's: the compare carried the |x| modifier);
  * "loose": the same with other selects on the mask too, or with one half only -- to be looked at by hand;
  * v_max_f64 x, x, x: the compiler quieting an operand ahead of a maximum or minimum of its own.
By source line when the listing carries .loc lines (the asm rule's compile line with -gline-tables-only added), else under None.
Default kernel: tl_frame_kernel<1, false, 2>, the one bench.py times."""
import re
import sys
from collections import Counter

path = sys.argv[1]
kern = sys.argv[2] if len(sys.argv) > 2 else "_Z15tl_frame_kernelILi1ELb0ELi2EEv8TlLaunch"
files = {}
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith(kern + ":"))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
for l in lines:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[int(m.group(1))] = m.group(3) or m.group(2)
ins = []        # (text, loc)
loc = None
for l in lines[start:end]:
    s = l.strip()
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
    if m:
        loc = "%s:%s" % (files.get(int(m.group(1)), m.group(1)).split("/")[-1], m.group(2))
        continue
    if not s or s.startswith(".") or s.startswith(";") or s.endswith(":"):
        continue
    ins.append((s.split(";")[0].strip(), loc))


def regs(op):
    """v[18:19] / |v[18:19]| / -v[1:2] -> (18, 19); else None"""
    m = re.search(r"v\[(\d+):(\d+)\]", op)
    return (int(m.group(1)), int(m.group(2))) if m else None


sites, selfmax, loose = Counter(), Counter(), Counter()
nsites = 0
for i, (t, lc) in enumerate(ins):
    m = re.match(r"v_max_f64(?:_e64)?\s+(\S+),\s*(\S+),\s*(\S+)", t)
    if m and m.group(2).rstrip(",") == m.group(3):
        selfmax[lc] += 1
    m = re.match(r"v_cmp_(gt|lt|ge|le|ngt|nlt|nge|nle)_f64(?:_e64|_e32)?\s+(.*)", t)
    if not m:
        continue
    ops = [o.strip() for o in m.group(2).split(",")]
    if len(ops) == 2:
        mask, a, b = "vcc", ops[0], ops[1]
    else:
        mask, a, b = ops[0], ops[1], ops[2]
    ra, rb = regs(a), regs(b)
    if not ra or not rb:
        continue
    # an absolute value's high half may have been made by a v_and_b32 just before
    alias = {}
    for t2, _ in ins[max(0, i - 6):i]:
        m2 = re.match(r"v_and_b32(?:_e32|_e64)?\s+v(\d+),\s*0x7fffffff,\s*v(\d+)", t2)
        if m2:
            alias[int(m2.group(1))] = int(m2.group(2))
    half = {ra[0]: "a", ra[1]: "a", rb[0]: "b", rb[1]: "b"}
    sel = []
    for t2, _ in ins[i + 1:i + 14]:
        if re.match(r"(v_cmp|v_cmpx)", t2) and (mask == "vcc" and (len(t2.split(",")) == 2 or " vcc" in t2.split(",")[0]) or t2.split()[1].rstrip(",") == mask):
            break
        m2 = re.match(r"v_cndmask_b32(?:_e32|_e64)?\s+v(\d+),\s*(\S+),\s*(\S+),\s*(\S+)", t2)
        if m2 and m2.group(4) == mask:
            srcs = []
            for g in (2, 3):
                mm = re.match(r"v(\d+)$", m2.group(g).rstrip(","))
                r = int(mm.group(1)) if mm else None
                r = alias.get(r, r)
                srcs.append(half.get(r))
            sel.append(tuple(srcs))
    good = [s for s in sel if set(s) == {"a", "b"}]
    if len(good) >= 2 and len(good) == len(sel):
        sites[lc] += 1
        nsites += 1
    elif len(good) >= 1:
        loose[lc] += 1
print("kernel", kern)
print("fp64 compare + 64-bit select between the compared values:", nsites)
for k, v in sorted(sites.items(), key=lambda kv: -kv[1]):
    print("   %4d  %s" % (v, k))
print("loose (a mask that also feeds other selects, or one half only):", sum(loose.values()))
for k, v in sorted(loose.items(), key=lambda kv: -kv[1]):
    print("   %4d  %s" % (v, k))
print("v_max_f64 x, x, x:", sum(selfmax.values()))
for k, v in sorted(selfmax.items(), key=lambda kv: -kv[1]):
    print("   %4d  %s" % (v, k))
allcmp = sum(1 for t, _ in ins if re.match(r"v_cmp_\w+_f64", t))
print("all v_cmp_*_f64:", allcmp, " v_max_f64:", sum(1 for t, _ in ins if t.startswith("v_max_f64")), " v_min_f64:", sum(1 for t, _ in ins if t.startswith("v_min_f64")),
      " v_cndmask_b32:", sum(1 for t, _ in ins if t.startswith("v_cndmask_b32")), " vector+scalar instructions:", len(ins))
