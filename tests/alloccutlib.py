"""Support for tests/test_alloc_cut_emu.py and tests/test_alloc_cut_gpu.py: a case set for the CLOSING ROUND of tl_allocate (csrc/mp2_alloc.h:
the round that does not fit as a whole is cut by key buckets before the lane-by-lane pass), the per-case path counters of the emulation
(tests/emu/mp2_alloc_cut_emu.cpp, compiled at first use into a temporary directory) and the bench-like frames
whose counters profiles/ab_alloc_cut.txt records.

The oracle is tests/probelib.py alloc_greedy, the reference's loop event by event.  What is restated HERE is only the round structure the
cases are placed on -- which events a round holds, their keys and prices, the window [lo, hi] and the bucket of each key, from the
definitions DESIGN.md section 4 states (b = (key - lo) >> sh, (hi - lo) >> sh <= 63) -- never a verdict: the replay decides where a budget is
put, alloc_greedy decides what the result must be.  `python tests/alloccutlib.py` prints the record of the bench-like frames."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

import probelib as P
from loudnesslib import GXX

ROOT = Path(__file__).resolve().parent.parent
U64 = np.uint64
I32 = np.int32
COUNTERS = ("PARTIAL", "FIRST", "EVENTS", "SERIAL", "PASS1", "PASS2", "DEGENERATE", "SMALL", "CUT0", "CUTLAST", "ONEBUCKET", "BELOW", "JOINTCUT", "ADMITTED")
K = {n: i for i, n in enumerate(COUNTERS)}
COVER = P.ALLOC_COVER
# what the emulation is built as: the text as it stands, the lane-by-lane pass alone (the parent's loop), and the four mutants
VARIANTS = {"cut": [], "serial": ["-DTL_CUT_PASSES=0"], "mutant1": ["-DTL_ALLOC_MUTANT=1"], "mutant2": ["-DTL_ALLOC_MUTANT=2"],
            "mutant3": ["-DTL_ALLOC_MUTANT=3"], "mutant4": ["-DTL_ALLOC_MUTANT=4"]}
# (holding a bucket's running sum against the room with `>=` for `>` is NO mutant: the cut then falls one occupied bucket early, and that
# bucket's cells get their exact sums from the lane-by-lane pass -- the same verdicts)
MUTANTS = {"mutant1": "`<` for `<=` in the bucket verdict: the cells of the cut's own bucket are refused without a sum of their own",
           "mutant2": "the lane-by-lane pass starts its sums at 0, not at the running sum of the buckets below the cut",
           "mutant3": "the non-paying lane of a joint pair adds the pair's price to the histogram a second time",
           "mutant4": "the shift one too small: bucket numbers above 63"}


def lib(variant="cut"):
    L = P._build("liballoccut_%s.so" % variant, GXX + VARIANTS[variant] + ["-shared", str(ROOT / "tests" / "emu" / "mp2_alloc_cut_emu.cpp"),
                                                                         str(ROOT / "odr-audioenc_amd" / "csrc" / "mp2_host.cpp"), "-lm"])
    L.alloc_cut_cases.argtypes = [C.c_long] + [C.c_void_p] * 6
    assert L.alloc_cut_ncounters() == len(COUNTERS)
    return L


def arrays(S):
    """the three input arrays of TLS_ALLOC (csrc/mp2_probe_stage.h), as tests/probelib.py run_stage lays them out"""
    n = S["tab"].size
    par = np.zeros((n, 8), dtype=I32)
    par[:, 0], par[:, 1], par[:, 2], par[:, 3], par[:, 4:6] = S["tab"], S["nch"], S["jsb"], S["call"], S["adb"]
    return [np.ascontiguousarray(x) for x in (S["smr"].transpose(0, 2, 1), S["scfsi"].transpose(0, 2, 1).astype(I32), par)]


def run_emu(L, S):
    """-> (rc, ba [n, 64], bits left [n], counters [n, len(COUNTERS)])"""
    n = S["tab"].size
    ins = arrays(S)
    ba, left, st = np.full(64 * n, -9, dtype=I32), np.full(n, -9, dtype=I32), np.zeros((n, len(COUNTERS)), dtype=np.int64)
    rc = L.alloc_cut_cases(n, P._ptr(ins[0]), P._ptr(ins[1]), P._ptr(ins[2]), P._ptr(ba), P._ptr(left), P._ptr(st))
    return rc, ba, left, st


def run_probe(fn, S):
    """fn = probe_stage of tests/emu/mp2_probe_emu.cpp or tlb_debug_probe_stage of the TEST library -> (rc, ba, bits left)"""
    n = S["tab"].size
    ins = arrays(S)
    ba, left = np.full(64 * n, -9, dtype=I32), np.full(n, -9, dtype=I32)
    rc = fn(P.STAGE["alloc"], n, P._ptr(ins[0]), P._ptr(ins[1]), P._ptr(ins[2]), P._ptr(ba), P._ptr(left))
    return rc, ba, left


# ---- the round structure of one case
def mnr_key(m):
    """tl_mnr_key (csrc/mp2_dbsum.h) from its comment: an order-preserving map of the double onto uint64, all ones from 999999.0 on"""
    m = np.asarray(m, dtype=np.float64)
    u = (m + 0.0).view(U64)
    k = np.where((u >> U64(63)) != 0, ~u, u | U64(1 << 63))
    return np.where(999999.0 > m, k, P.ALL1)


def rounds_of(tab, nch, jsb, smr, scfsi, max_spent=P.ALLOC_MAX_ADB):
    """The rounds of one case while everything fits: per round dict(lo, M: the smallest second key of the round before (0: none) and of this one,
    spent: the bits of the rounds before, key / price / lane / joint: the round's paying events in lane order).  -> (rounds, bbal)"""
    T = P._alloc_tables()
    line, maxa, live, joint, bbal = (x[0] for x in P._alloc_geometry(np.array([tab]), np.array([nch]), np.array([jsb])))
    lv = np.arange(17)
    step = T["step"][line][:, np.minimum(lv, 15)]                          # [32, 17]
    snr = np.where(lv[None, :] == 0, T["snr"][0], T["snr"][step])
    b12 = np.where(lv[None, :] == 0, 0, T["bits12"][step])
    keys = mnr_key(snr[None, :, :] - np.asarray(smr, dtype=np.float64)[:, :, None])
    keys = np.where(live[:, :, None] & (lv[None, None, :] < maxa[None, :, None]), keys, P.ALL1)      # [2, 32, 17]: the key of the step from level b
    sfs = 6 * P.SFS_PER_SCFSI[np.asarray(scfsi, dtype=np.int64)]
    first = b12[None, :, 1] + 2 + sfs + np.where(joint[None, :], 2 + sfs[::-1], 0)
    ba = np.zeros((2, 32), dtype=np.int64)
    lane = 2 * np.arange(32)[None, :] + np.arange(2)[:, None]
    out, spent, lo = [], 0, 0
    take = lambda a, b: np.take_along_axis(a, b[:, :, None], axis=2)[:, :, 0]
    while spent <= max_spent and len(out) < 64:
        k1, k2 = take(keys, ba), take(keys, np.minimum(ba + 1, 16))
        keff, k2eff = k1.copy(), k2.copy()
        keff[:, joint], k2eff[:, joint] = k1[:, joint].min(axis=0), k2[:, joint].min(axis=0)
        M = int(k2eff.min())
        inb = keff < U64(M)
        if not inb.any():
            break
        pay = inb & ~(joint[None, :] & (np.arange(2)[:, None] == 1))
        bsb = np.broadcast_to(np.arange(32)[None, :], (2, 32))
        price = np.where(ba == 0, first, take(np.broadcast_to(b12[None], (2, 32, 17)), np.minimum(ba + 1, 16)) - take(np.broadcast_to(b12[None], (2, 32, 17)), ba))
        o = np.argsort(lane[pay])
        out.append(dict(lo=lo, M=M, spent=spent, key=[int(x) for x in keff[pay][o]], price=[int(x) for x in price[pay][o]], lane=[int(x) for x in lane[pay][o]],
                        joint=[bool(x) for x in joint[bsb[pay]][o]]))
        spent += int(price[pay].sum())
        ba = ba + inb
        lo = M
    return out, int(bbal)


def buckets_of(r):
    """the first bucket pass of a round from its definition -> (bucket of each event, sum of each of the 64 buckets), or None for a window of one key"""
    lo, hi = r["lo"], r["M"] - 1
    if hi <= lo:
        return None
    sh = max(0, (hi - lo).bit_length() - 6)
    b = [(k - lo) >> sh for k in r["key"]]
    assert all(0 <= x <= 63 for x in b), "a key outside the window"
    h = [0] * 64
    for x, p in zip(b, r["price"]):
        h[x] += p
    return b, h


# ---- the set
EXTRA_SMR = ("keys a few ulps apart", "every cell in the first round", "two clusters")
KINDS = ("cut in bucket 0", "cut in the last occupied bucket", "room = a bucket's running sum", "room one bit short of a bucket's running sum", "one bucket", "all keys equal",
         "first round", "window over negative and positive MNR", "joint pair at the cut, tied with a lower lane", "joint pair at the cut, tied with a higher lane",
         "round of 1 event", "round of 54 events")
_sets = {}


def _smr(g, kind, tab, T):
    if kind == "keys a few ulps apart":                                    # one bucket however the window is cut: the second pass and the lane-by-lane pass get them all
        s0 = float(g.uniform(-10.0, 30.0))
        return s0 + g.integers(0, 64, (2, 32)) * 2.0 ** -44, g.integers(0, 4, (2, 32))
    if kind == "every cell in the first round":                            # a spread below the smallest first SNR step
        return float(g.uniform(-10.0, 30.0)) + g.uniform(0.0, 0.5, (2, 32)), g.integers(0, 4, (2, 32))
    if kind == "two clusters":
        return np.where(g.random((2, 32)) < 0.5, 4.0, 11.0) + g.uniform(0.0, 0.05, (2, 32)), g.integers(0, 4, (2, 32))
    return P._alloc_smr(g, kind, tab, T)


def _rooms(g, r):
    """budgets inside round r, (room, why) with 0 <= room < the round's total: the places the cut's arithmetic can go wrong"""
    tot, n = sum(r["price"]), len(r["price"])
    out = [(int(g.integers(0, tot)), "random")]
    order = sorted(range(n), key=lambda i: r["key"][i])
    bk = buckets_of(r)
    if bk is not None:
        b, h = bk
        occ = [x for x in range(64) if h[x]]
        cum = np.cumsum(h)
        if h[0]:
            out.append((int(g.integers(0, h[0])), "bucket 0"))
        out.append((int(g.integers(cum[occ[-1]] - h[occ[-1]], tot)), "last bucket"))
        for x in occ[:-1][:: max(1, len(occ) // 3)]:
            out += [(int(cum[x]), "bucket sum"), (int(cum[x]) - 1, "bucket sum - 1")]
    # a group of tied events: just below it, one bit short of all of it, all of it
    below, i = 0, 0
    groups = []
    while i < n:
        j = i
        while j < n and r["key"][order[j]] == r["key"][order[i]]:
            j += 1
        grp = sum(r["price"][order[q]] for q in range(i, j))
        if j - i > 1:
            groups.append((below, grp))
        below += grp
        i = j
    for below, grp in groups[:: max(1, len(groups) // 2)]:
        out += [(below, "tie: none"), (below + grp - 1, "tie: one short"), (below + grp, "tie: all")]
    if n == 1:
        out += [(0, "one event"), (tot - 1, "one event")]
    return [(room, why) for room, why in out if 0 <= room < tot]


def cut_set():
    """-> dict(tab, nch, jsb, call, adb [n, 2], smr, scfsi [n, 2, 32], names, facts: per case what the replay says of its closing round)"""
    if "cut" in _sets:
        return _sets["cut"]
    T = P._alloc_tables()
    g = np.random.default_rng(62)
    cfgs = [(t, 1, int(T["sblimit"][t])) for t in range(5)] + [(t, 2, j) for t in range(5) for j in sorted({4, 8, 12, 16, int(T["sblimit"][t])})]
    cases = []
    for t, nch, jsb in cfgs:
        for kind in P.ALLOC_SMR_KINDS + EXTRA_SMR:
            if kind == "upper channel first" and not (nch == 2 and jsb < T["sblimit"][t]):
                kind = "keys a few ulps apart"
            smr, sel = _smr(g, kind, t, T)
            smr = np.clip(smr, -1000.0, 1000.0)
            R, bbal = rounds_of(t, nch, jsb, smr, sel)
            if not R:
                continue
            pick = {0, int(g.integers(0, len(R))), int(g.integers(0, len(R))), len(R) - 1}
            pick |= {i for i, r in enumerate(R) if len(r["price"]) == 1 or len(r["price"]) == 54}
            for i in sorted(pick):
                r = R[i]
                rooms = _rooms(g, r)
                if i == 0 and len(pick) > 1:
                    rooms = rooms[:4]
                for room, why in rooms:
                    adb = bbal + 48 + r["spent"] + room
                    if adb <= P.ALLOC_MAX_ADB:
                        cases.append((t, nch, jsb, adb, smr, sel, "%s; round %d of %d events, room %d (%s)" % (kind, i, len(r["price"]), room, why), r, room))
    col = lambda i, dt: np.array([c[i] for c in cases], dtype=dt)
    S = dict(tab=col(0, I32), nch=col(1, I32), jsb=col(2, I32), call=np.zeros(len(cases), dtype=I32), adb=np.stack([col(3, I32), np.zeros(len(cases), dtype=I32)], axis=1),
             smr=col(4, np.float64), scfsi=col(5, I32), names=[c[6] for c in cases], facts=[closing_facts(c[7], c[8]) for c in cases])
    assert len(cases) <= 8192
    _sets["cut"] = S
    return S


def closing_facts(r, room):
    """what the replay says of a closing round r at `room` bits: the conditions of KINDS that the path counters cannot tell"""
    n = len(r["price"])
    f = dict(events=n, first=r["spent"] == 0, spans_zero=r["lo"] < (1 << 63) <= r["M"] - 1, all_equal=n > 1 and len(set(r["key"])) == 1,
             on_sum=False, short_of_sum=False, joint_tie_lower=False, joint_tie_higher=False)
    # the rule of the partial round: an event stays iff the prices of the round's events with a key <= its own fit the room
    f["admitted"] = sum(1 for k in r["key"] if sum(p for k2, p in zip(r["key"], r["price"]) if k2 <= k) <= room)
    bk = buckets_of(r)
    if bk is not None:
        cum = np.cumsum(bk[1])
        occ = [x for x in range(64) if bk[1][x]]
        f["on_sum"] = any(room == cum[x] for x in occ)
        f["short_of_sum"] = any(room == cum[x] - 1 for x in occ)
    # the tie group the cut falls into or ends on: a joint pair's event in it, tied with an event of a lower / a higher lane
    for i in range(n):
        if not r["joint"][i]:
            continue
        same = [j for j in range(n) if j != i and r["key"][j] == r["key"][i]]
        if not same:
            continue
        below = sum(p for k, p in zip(r["key"], r["price"]) if k < r["key"][i])
        grp = sum(p for k, p in zip(r["key"], r["price"]) if k == r["key"][i])
        if below <= room <= below + grp:
            f["joint_tie_lower"] |= any(r["lane"][j] < r["lane"][i] for j in same)
            f["joint_tie_higher"] |= any(r["lane"][j] > r["lane"][i] for j in same)
    return f


def coverage(S, st, serial_limit):
    """KINDS -> number of cases, from the emulation's counters of each case (which branch ran, what was left to the lane-by-lane pass) and, for what
    the counters cannot tell, from the replay's facts.  A condition on the bucket passes counts only cases whose first pass RAN."""
    F = S["facts"]
    fact = lambda k: np.array([f[k] for f in F])
    p1 = (st[:, K["PARTIAL"]] == 1) & (st[:, K["PASS1"]] == 1)
    many = fact("events") > serial_limit
    return {
        "cut in bucket 0": int((p1 & (st[:, K["CUT0"]] == 1)).sum()),
        "cut in the last occupied bucket": int((p1 & (st[:, K["CUTLAST"]] == 1) & (st[:, K["ONEBUCKET"]] == 0)).sum()),
        "room = a bucket's running sum": int((p1 & fact("on_sum")).sum()),
        "room one bit short of a bucket's running sum": int((p1 & fact("short_of_sum")).sum()),
        "one bucket": int((p1 & (st[:, K["ONEBUCKET"]] == 1)).sum()),
        "all keys equal": int((p1 & fact("all_equal") & (st[:, K["SERIAL"]] == st[:, K["EVENTS"]])).sum()),
        "first round": int((p1 & (st[:, K["FIRST"]] == 1)).sum()),
        "window over negative and positive MNR": int((p1 & fact("spans_zero")).sum()),
        "joint pair at the cut, tied with a lower lane": int((p1 & (st[:, K["JOINTCUT"]] == 1) & fact("joint_tie_lower")).sum()),
        "joint pair at the cut, tied with a higher lane": int((p1 & (st[:, K["JOINTCUT"]] == 1) & fact("joint_tie_higher")).sum()),
        "round of 1 event": int(((st[:, K["PARTIAL"]] == 1) & (st[:, K["EVENTS"]] == 1)).sum()),
        "round of 54 events": int((p1 & (st[:, K["EVENTS"]] == 54)).sum()),
        "second pass": int((st[:, K["PASS2"]] == 1).sum()),
        "short round: no pass": int(((st[:, K["PARTIAL"]] == 1) & (st[:, K["SMALL"]] == 1) & ~many).sum()),
    }


def check(S, ba, left):
    """a run's results against alloc_greedy, word for word -> None or a message naming the case"""
    return P.alloc_check(S, ba, left)


def check_rule(S, st):
    """The closing round admits exactly the events the partial round's rule admits (the replay's count), no fewer: the event-by-event loop
    behind it would make up for a round cut short, so the result's words alone do not see one.  -> None or a message naming the case"""
    want = np.array([f["admitted"] for f in S["facts"]])
    bad = np.flatnonzero(st[:, K["ADMITTED"]] != want)
    if bad.size:
        c = int(bad[0])
        return "case %d (%s): the closing round admitted %d events, the rule admits %d (%d cases differ)" % (c, S["names"][c], st[c, K["ADMITTED"]], want[c], bad.size)
    return None


# ---- the bench-like frames (profiles/ab_alloc_cut.txt): the oracle's SMR and scfsi taps of bench.py's own signals
def bench_like(seeds=range(12), frames=range(2, 12)):
    import oraclelib as O
    from pcmgen import gen_pcm
    T = P._alloc_tables()
    smr, sel, adb, want = [], [], [], []
    nf = max(frames) + 1
    for s in seeds:
        e = O.OracleEncoder(samplerate=48000, mode="s", kbps=128, psy=1)
        pcm = gen_pcm(s, 0, 0, nf)
        for f in range(nf):
            e.encode(pcm[f])
            if f not in frames:
                continue
            t = e.taps()
            line = T["line"][0]
            ba_ = t["bit_alloc"].astype(np.int64)
            livec = np.arange(32)[None, :] < T["sblimit"][0]
            spent = np.where(livec & (ba_ > 0), T["bits12"][T["step"][np.where(line == 255, 0, line)[None, :], ba_]] + 2 + 6 * P.SFS_PER_SCFSI[t["scfsi"].astype(np.int64)], 0).sum()
            bbal = int(2 * T["nbal"][line[: T["sblimit"][0]]].sum())
            smr.append(t["smr"]); sel.append(t["scfsi"]); adb.append(int(t["adb_left"] + spent + bbal + 48)); want.append(ba_)
        e.close()
    n = len(adb)
    S = dict(tab=np.zeros(n, dtype=I32), nch=np.full(n, 2, dtype=I32), jsb=np.full(n, int(T["sblimit"][0]), dtype=I32), call=np.zeros(n, dtype=I32),
             adb=np.stack([np.array(adb, dtype=I32), np.zeros(n, dtype=I32)], axis=1), smr=np.array(smr, dtype=np.float64), scfsi=np.array(sel, dtype=I32),
             names=["bench-like frame %d" % i for i in range(n)], taps_ba=np.array(want))
    return S


def bench_like_record():
    S = bench_like()
    lines = []
    for v in ("serial", "cut"):
        rc, ba, left, st = run_emu(lib(v), S)
        assert rc == 0 and check(S, ba, left) is None
        assert (ba.reshape(-1, 32, 2).transpose(0, 2, 1) == np.where(np.arange(32) < 27, S["taps_ba"], 0)).all(), "not the reference's bit_alloc"
        m = lambda k: "%5.2f (%d..%d)" % (st[:, K[k]].mean(), st[:, K[k]].min(), st[:, K[k]].max())
        lines.append("%-6s frames %d, partial-round branch %d, events of the closing round %s, left to the lane-by-lane pass %s, first passes %d, second passes %d, keys outside the window %d"
                     % (v, st.shape[0], st[:, K["PARTIAL"]].sum(), m("EVENTS"), m("SERIAL"), st[:, K["PASS1"]].sum(), st[:, K["PASS2"]].sum(), st[:, K["BELOW"]].sum()))
    return lines


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    print("\n".join(bench_like_record()))
