"""The node's tick deadline on the GPU (include/toolame_batch.h, TICK DEADLINE; csrc/tlb_node.cpp).

A shard whose tick does not complete is held up by nothing a healthy GPU does, so the stall is injected on the fault-injection TEST build
(odr-audioenc_amd/libtoolame_dab_hip_fi.so, csrc/tlb_debug.h): tlb_debug_node_stall_next holds ONE shard's host thread after its tick
has completed on the device -- no kernel spins, no event is left incomplete, the device stays idle and healthy.  devices = (0, 0, 0) and
the nine mixed streams of test_node_fault_gpu.py's tick-plane case (psy 0-4, mono and stereo, 16 / 24 / 48 kHz).

Deadline and stall are derived here, not fixed in advance: an undisturbed node without a deadline is driven first (the existing code
path), D = max(250 ms, 10 x its slowest run()), S = 4 x D.  Ticks are paced 24 ms apart, one DAB frame, as the real loop is.  A healthy
shard going late is a failure, not a retry."""
import ctypes as C
import time

import numpy as np
import pytest

import oraclelib as O
from pcmgen import gen_pcm

pytestmark = pytest.mark.gpu

STREAMS = [(48000, "s", 128, 1), (48000, "j", 128, 3), (24000, "m", 64, 1), (48000, "s", 192, 2), (48000, "m", 96, 4), (48000, "m", 96, 4),
           (16000, "m", 32, 3), (48000, "s", 128, 1), (48000, "j", 160, 3)]
NS = len(STREAMS)
POOL = 64                       # distinct input frames per stream; tick f reads frame f % POOL
PERIOD = 0.024                  # one DAB frame
K = 3                           # the tick at which shard 1 stalls
LATE, HIP, ARG = 19, 17, 18


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def FI(M):
    if not M.FAULT_LIB_PATH.exists():
        M.build()
    return M.load_fault_library()


@pytest.fixture(scope="module")
def cfgs(M):
    return [M.StreamConfig(samplerate=r, mode=m, bitrate=k, psy_model=p) for r, m, k, p in STREAMS]


@pytest.fixture(scope="module")
def pool():
    """int16 [POOL][NS][2304]: every stream's interleaved frame per tick"""
    per = [gen_pcm(8600 + s, (0, 7, 5, 4)[s % 4], 0, POOL) for s in range(NS)]
    return np.stack([np.stack([per[s][f].T.reshape(-1) for s in range(NS)]) for f in range(POOL)])


def _inp(pool, f):
    return pool[f % POOL]


def _planar(inter_s, c):
    T = inter_s.shape[0]
    if c.mode == "m":
        return np.repeat(inter_s[:, None, :1152], 2, axis=1)
    return inter_s.reshape(T, 1152, 2).transpose(0, 2, 1)


def _oracle_frames(pool, ticks, s, c):
    """the oracle's frames of stream s over the inputs of `ticks` (every rate here has frames of one length)"""
    inter = np.stack([_inp(pool, f)[s] for f in ticks])
    b, _ = O.oracle_stream(_planar(inter, c), samplerate=c.samplerate, mode=c.mode, kbps=c.bitrate, psy=c.psy_model)
    n = len(ticks)
    assert n and len(b) % n == 0, (s, len(b), n)
    L = len(b) // n
    return [b[i * L:(i + 1) * L] for i in range(n)]


def _snap(nd):
    return [(nd.frame(s), nd.peaks(s), nd.silence_ms(s)) for s in range(NS)]


def _pace(t0, f):
    dt = t0 + PERIOD * (f + 1) - time.perf_counter()
    if dt > 0:
        time.sleep(dt)


def _undisturbed(M, lib, cfgs, pool, T, paced=True):
    """the existing code path: no deadline, run() per tick, finish -> (snaps of T ticks + finish, run() times in ms)"""
    nd = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames", ngroups=2, lib=lib)
    out, ms = [], []
    t0 = time.perf_counter()
    for f in range(T):
        nd.set_pcm(_inp(pool, f))
        a = time.perf_counter()
        nd.run()
        ms.append((time.perf_counter() - a) * 1e3)
        out.append(_snap(nd))
        if paced:
            _pace(t0, f)
    nd.finish()
    out.append(_snap(nd))
    nd.close()
    return out, ms


@pytest.fixture(scope="module")
def budget(M, FI, cfgs, pool):
    _, ms = _undisturbed(M, FI, cfgs, pool, 40)
    slowest = max(ms[1:])                                               # (the first run pays for the first launch of every kernel)
    D = max(250.0, 10.0 * slowest)
    S = 4.0 * D
    print(f"\nnode deadline budget: slowest undisturbed run() {slowest:.2f} ms (first {ms[0]:.2f} ms), D = {D:.1f} ms, S = {S:.1f} ms")
    return dict(slowest=slowest, D=D, S=S)


def _expected_delivered(frames, accepted, dropped):
    """the i-th accepted tick retires frame i-1, finish the last; frames retired at dropped ticks are never shown"""
    out = [frames[i - 1] for i, step in enumerate(accepted) if i >= 1 and step not in dropped]
    return b"".join(out) + frames[len(accepted) - 1]


def _check_healthy(got, want, nd_dl, pool, cfgs, blocks, T):
    for g in (0, 2):
        assert nd_dl[g]["late_events"] == 0 and nd_dl[g]["state"] == 0, (g, nd_dl[g])
        f0, n = blocks[g]
        for s in range(f0, f0 + n):
            for f in range(T + 1):
                assert got[f][s] == want[f][s], (f, s)
            fr = _oracle_frames(pool, range(T), s, cfgs[s])
            assert b"".join(got[f][s][0] for f in range(T + 1)) == b"".join(fr), s


def _drive(M, FI, cfgs, pool, budget, pipelined, stall_rc=0):
    """shard 1 stalls once (S) in the wait of tick K; the loop runs until it is back (rejoined, or broken + restarted) plus 5 ticks"""
    D, S = budget["D"], budget["S"]
    nd = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames", ngroups=2, lib=FI, deadline_ms=D)
    f1, n1 = nd.blocks[1]
    got, rcs, late_seen, back_at, restarted_at = [], {}, [], None, None
    t0 = time.perf_counter()
    t_stall = None
    submitted, stop_at, t = 0, None, 0

    def submit():
        nonlocal submitted
        nd.set_pcm(_inp(pool, submitted))
        nd.submit()
        submitted += 1

    if pipelined:
        submit()
    while True:
        if pipelined:
            if stop_at is None or submitted < stop_at:
                submit()
        else:
            nd.set_pcm(_inp(pool, t))
            submitted += 1
        if t == K:
            nd.stall_next(1, 1, S, stall_rc)
            t_stall = time.perf_counter()
        try:
            nd.wait() if pipelined else nd.run()
            rcs[t] = 0
        except M.ToolameError as e:
            rcs[t] = e.code
        got.append(_snap(nd))
        st = nd.shard_status(1)["state"]
        dl = nd.shard_deadline(1)
        if t_stall is not None and back_at is None:
            if st == 2:
                late_seen.append(t)
                assert nd.pcm(f1) is None and all(got[t][s] == (b"", None, 0) for s in range(f1, f1 + n1)), t
            elif stall_rc == 0 and dl["rejoins"] == 1:
                back_at = t
                assert all(got[t][s] == (b"", None, 0) for s in range(f1, f1 + n1)), t       # back, but not in the step just waited for
            elif stall_rc and st == 1:
                back_at = t
                assert rcs[t] == stall_rc and nd.shard_status(1)["last_err"] == stall_rc, (t, rcs[t])
                nd.shard_restart(1)                                     # the run() loop: no tick in flight
                restarted_at = t + 1
            if back_at is not None:
                stop_at = submitted + (5 if not pipelined else 6)
            assert time.perf_counter() - t_stall < 10 * S / 1e3, "shard 1 did not come back within 10 x S"
        t += 1
        if not pipelined:
            _pace(t0, t - 1)
            if stop_at is not None and t >= stop_at:
                break
        else:
            _pace(t0, t - 1)
            if t == submitted:
                break
    T = t
    nd.finish()
    got.append(_snap(nd))
    per, _ = nd.counters()
    dls = [nd.shard_deadline(g) for g in range(3)]
    nd.close()
    return dict(got=got, rcs=rcs, late_seen=late_seen, back_at=back_at, restarted_at=restarted_at, T=T, per=per, dls=dls, n1=n1)


def _blocks(M, cfgs):
    return M.node_partition(len(cfgs), 3)


@pytest.mark.parametrize("pipelined", [False, True], ids=["run_loop", "submit_submit_wait"])
def test_stalled_shard_goes_late_and_rejoins_on_its_own(M, FI, cfgs, pool, budget, pipelined):
    """a. / b.  Shard 1 stalls once (rc 0) in the wait of tick K.  Shards 0 and 2 match an undisturbed node and the oracle on every tick
    and after finish and are never late; the call at tick K returns TLB_ERR_LATE; shard 1 reads LATE with empty accessors until it comes
    back by itself (no restart), then delivers the oracle's frames of the inputs it accepted with those retired at dropped ticks removed."""
    r = _drive(M, FI, cfgs, pool, budget, pipelined)
    T, got, dl1, per = r["T"], r["got"], r["dls"][1], r["per"]
    print(f"{'pipelined' if pipelined else 'run loop'}: T {T}, late at {r['late_seen'][:1]}..{r['late_seen'][-1:]}, back at {r['back_at']}, "
          f"shard 1 {dl1}, D {budget['D']:.1f} ms, S {budget['S']:.1f} ms, slowest healthy run {budget['slowest']:.2f} ms")
    assert r["back_at"] is not None
    assert r["rcs"][K] == LATE and all(rc == 0 for t, rc in r["rcs"].items() if t != K), r["rcs"]
    assert r["late_seen"] and r["late_seen"][0] == K
    want, _ = _undisturbed(M, FI, cfgs, pool, T, paced=False)
    blocks = _blocks(M, cfgs)
    _check_healthy(got, want, r["dls"], pool, cfgs, blocks, T)
    # the record of the episode
    rj = dl1["last_rejoin_step"]
    assert dl1["state"] == 0 and dl1["late_events"] == 1 and dl1["rejoins"] == 1 and dl1["last_late_step"] == K
    assert dl1["dropped_steps"] == (2 if pipelined else 1)
    assert rj == r["back_at"] + (2 if pipelined else 1)
    assert per[1]["steps"] + dl1["dropped_steps"] + dl1["missed_steps"] == T, (per[1], dl1, T)
    assert per[1]["frames"] == r["n1"] * per[1]["steps"]
    assert dl1["worst_overrun_ms"] > 0
    # shard 1: silent from K until the first step it took part in after coming back; then the frames of the inputs it accepted
    accepted = list(range(0, K + (2 if pipelined else 1))) + list(range(rj, T))
    dropped = {K, K + 1} if pipelined else {K}
    f1, n1 = blocks[1]
    for s in range(f1, f1 + n1):
        for f in range(K):
            assert got[f][s] == want[f][s], (f, s)
        for f in range(K, rj):
            assert got[f][s] == (b"", None, 0), (f, s)
        fr = _oracle_frames(pool, accepted, s, cfgs[s])
        assert b"".join(got[f][s][0] for f in range(T + 1)) == _expected_delivered(fr, accepted, dropped), s


def test_late_shard_that_returns_an_error_breaks_and_restarts(M, FI, cfgs, pool, budget):
    """c.  The stall returns TLB_ERR_HIP: shard 1 goes LATE, becomes BROKEN at the first poll after the sleep (that call returns the
    code); restarted it is a fresh encoder, oracle from that tick on.  Shards 0 and 2 are undisturbed throughout."""
    r = _drive(M, FI, cfgs, pool, budget, False, stall_rc=HIP)
    T, got, dl1 = r["T"], r["got"], r["dls"][1]
    print(f"late then broken: T {T}, broken at {r['back_at']}, restarted at {r['restarted_at']}, shard 1 {dl1}")
    assert r["back_at"] is not None and r["rcs"][K] == LATE and r["rcs"][r["back_at"]] == HIP
    assert all(rc == 0 for t, rc in r["rcs"].items() if t not in (K, r["back_at"])), r["rcs"]
    assert dl1["late_events"] == 1 and dl1["rejoins"] == 0 and dl1["state"] == 0
    want, _ = _undisturbed(M, FI, cfgs, pool, T, paced=False)
    blocks = _blocks(M, cfgs)
    _check_healthy(got, want, r["dls"], pool, cfgs, blocks, T)
    f1, n1 = blocks[1]
    ra = r["restarted_at"]
    for s in range(f1, f1 + n1):
        for f in range(K, ra):
            assert got[f][s] == (b"", None, 0), (f, s)
        fr = _oracle_frames(pool, range(ra, T), s, cfgs[s])
        assert b"".join(got[f][s][0] for f in range(ra, T + 1)) == b"".join(fr), s


def test_deadline_on_a_healthy_node_changes_nothing(M, cfgs, pool, budget):
    """d.  100 unpaced ticks with the deadline set: byte for byte the node without it; nobody late."""
    want, _ = _undisturbed(M, None, cfgs, pool, 100, paced=False)
    nd = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames", ngroups=2, deadline_ms=budget["D"])
    got = []
    for f in range(100):
        nd.set_pcm(_inp(pool, f))
        nd.run()
        got.append(_snap(nd))
    nd.finish()
    got.append(_snap(nd))
    dls = [nd.shard_deadline(g) for g in range(3)]
    nd.close()
    assert got == want
    assert all(d["late_events"] == 0 and d["missed_steps"] == 0 and d["dropped_steps"] == 0 and d["state"] == 0 for d in dls), dls


def test_deadline_rules(M, FI, cfgs, pool, budget):
    """e.  set_deadline_ms refuses a BATCH node, a negative value and a call with a step in flight; a late shard's restart, per-stream
    calls and tlb_node_pcm answer TLB_ERR_LATE / NULL; tlb_node_parallel does not call fn for it; finish skips it."""
    nb = M.Node(cfgs[:3], devices=(0,), plane="batch")
    assert nb.L.tlb_node_set_deadline_ms(nb.h, 100.0) == ARG
    nb.close()
    nd = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames", ngroups=2, lib=FI)
    L = nd.L
    assert L.tlb_node_set_deadline_ms(nd.h, -1.0) == ARG
    nd.set_pcm(_inp(pool, 0))
    nd.submit()
    assert L.tlb_node_set_deadline_ms(nd.h, budget["D"]) == ARG             # a step in flight
    nd.wait()
    nd.set_deadline_ms(budget["D"])
    f1, n1 = nd.blocks[1]
    nd.set_pcm(_inp(pool, 1))
    nd.stall_next(1, 1, budget["S"], 0)
    with pytest.raises(M.ToolameError) as e:
        nd.run()
    assert e.value.code == LATE and nd.shard_status(1)["state"] == 2
    assert nd.shard_deadline(1)["state"] == 2
    assert L.tlb_node_shard_restart(nd.h, 1, -1) == LATE
    assert L.tlb_node_stream_reset(nd.h, f1) == LATE
    assert L.tlb_node_stream_reconfigure(nd.h, f1, M.toolame._config_array([cfgs[f1]])) == LATE
    assert L.tlb_node_stream_finish(nd.h, f1, (C.c_uint8 * 2048)(), 2048) == -LATE
    assert L.tlb_node_set_gain_db(nd.h, f1, -3.0) == LATE
    assert nd.pcm(f1) is None and nd.frame(f1) == b"" and nd.peaks(f1) is None
    assert nd.pcm(nd.blocks[0][0]) is not None and nd.pcm(nd.blocks[2][0]) is not None
    seen = []
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int)
    cb = CB(lambda ctx, g, first, n: seen.append(g))
    assert L.tlb_node_parallel(nd.h, cb, None) == 0
    assert sorted(seen) == [0, 2]
    assert L.tlb_node_finish(nd.h) == 0                                      # shards 0 and 2 finish; the late one is skipped
    assert nd.frame(f1) == b"" and nd.shard_status(1)["state"] == 2
    assert all(nd.frame(s) for s in range(nd.blocks[0][0], nd.blocks[0][0] + nd.blocks[0][1]))
    t = time.perf_counter()
    nd.close()                                                              # waits for the late job (the stall) without a limit
    print(f"destroy waited {1e3 * (time.perf_counter() - t):.0f} ms for the late shard")
