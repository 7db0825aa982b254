"""Ingest with short reads on the GPU (csrc/toolame_ingest.hip, tlb_tick_* / tlb_node_* with short reads enabled): the device against the
lane-loop emulation byte for byte with the `valid` array and without it, a tick object with short reads against one fed the stretched PCM
as full reads, the alternation rule of the valid array, the node's per-stream accessors, and a tick object that never enables the feature."""
import shutil

import numpy as np
import pytest

import ingestlib as I
from pcmgen import gen_pcm

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")]

MIX = [(48000, "s", 128, 1), (48000, "m", 64, 1), (24000, "m", 64, 1), (48000, "j", 128, 3), (16000, "s", 64, 3), (32000, "m", 64, 1),
       (44100, "s", 128, 1), (24000, "j", 64, 1), (48000, "m", 96, 0), (48000, "s", 192, 1), (22050, "m", 32, 1)]
GAINS = [0.0, 0.0, -3.5, 6.0, 0.0, 2.25, -12.0, 0.0, 0.5, 0.0, 3.0]


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return I.IngestEmu(I.build_emu(tmp_path_factory.mktemp("ingestemu")))


def _cfgs(M, streams):
    return [M.StreamConfig(samplerate=r, mode=m, bitrate=k, psy_model=p) for r, m, k, p in streams]


def _nch(streams):
    return [1 if m == "m" else 2 for _, m, _, _ in streams]


def test_device_equals_emulation(M, emu):
    """a mixed batch (stereo and mono, six rates, gains), random `valid` that includes every fixture value and values out of range, junk
    behind `valid`: planar PCM, peaks and both underrun counters of the device equal the emulation's byte for byte, in ragged calls"""
    cfgs, nch, ns = _cfgs(M, MIX), _nch(MIX), len(MIX)
    fx = I.fixture()[0]
    nf = 2 * ((len(fx) + ns - 1) // ns) + 6
    rng = np.random.default_rng(3)
    inter = rng.integers(-32768, 32768, size=(nf, ns, 2 * I.FRAMES), dtype=np.int64).astype(np.int16)
    valid = rng.choice(np.concatenate([fx, [1152] * 60, [-1, 1153, 2000, -(1 << 31), (1 << 31) - 1]]), size=(nf, ns)).astype(np.int32)
    flat = valid.reshape(-1)
    flat[rng.permutation(flat.size)[:len(fx)]] = fx                 # every fixture value at least once
    assert set(int(v) for v in fx) <= set(int(v) for v in flat)
    b = M.Batch(cfgs)
    for s, g in enumerate(GAINS):
        b.set_gain_db(g, s)
    want_pcm, want_pk = emu.ingest(inter, valid, nch, GAINS)
    ms, n = np.zeros(ns, np.uint32), np.zeros(ns, np.uint32)
    want_ms, want_n = np.zeros(ns, np.uint32), np.zeros(ns, np.uint32)
    pos = 0
    for cut in (1, 7, 3, 2, 1, nf - 14):
        pcm, pk = b.ingest(inter[pos:pos + cut], valid[pos:pos + cut])
        assert pcm.tobytes() == want_pcm[pos:pos + cut].tobytes() and pk.tobytes() == want_pk[pos:pos + cut].tobytes(), pos
        b.underrun(valid[pos:pos + cut], ms, n)
        emu.underrun(valid[pos:pos + cut], [r for r, _, _, _ in MIX], nch, want_ms, want_n)
        assert np.array_equal(ms, want_ms) and np.array_equal(n, want_n), pos
        pos += cut
    assert pos == nf and n.sum() > 0
    # no array, and an array of full reads: the existing kernel's output
    a0, p0 = b.ingest(inter[:5])
    a1, p1 = b.ingest(inter[:5], np.full((5, ns), 1152, np.int32))
    a2, p2 = b.ingest(inter[:5], np.full((5, ns), 2000, np.int32))
    assert a0.tobytes() == a1.tobytes() == a2.tobytes() and p0.tobytes() == p1.tobytes() == p2.tobytes()
    b.close()


def test_device_without_the_array_equals_emulation(M, emu):
    """the same mixed batch (stereo and mono, six rates, gains of 0 dB and others), 3 frames, no `valid` array: tl_ingest_kernel's planar
    PCM and peaks equal the emulation's byte for byte, and tl_ingest_valid_kernel's with every slot at 1152"""
    cfgs, nch, ns, nf = _cfgs(M, MIX), _nch(MIX), len(MIX), 3
    rng = np.random.default_rng(31)
    inter = rng.integers(-32768, 32768, size=(nf, ns, 2 * I.FRAMES), dtype=np.int64).astype(np.int16)
    inter[0, 0, :8] = [32767, -32768, 0, 1, -1, 12345, -12345, 2]
    inter[1, 4] = 0                                                  # a silent stereo slot and a silent mono one: peaks (0, 0)
    inter[2, 1, :I.FRAMES] = 0
    b = M.Batch(cfgs)
    for s, g in enumerate(GAINS):
        b.set_gain_db(g, s)
    want_pcm, want_pk = emu.ingest(inter, None, nch, GAINS)
    pcm, pk = b.ingest(inter)
    assert pcm.tobytes() == want_pcm.tobytes() and pk.tobytes() == want_pk.tobytes()
    pcm_v, pk_v = b.ingest(inter, np.full((nf, ns), 1152, np.int32))
    assert pcm_v.tobytes() == pcm.tobytes() and pk_v.tobytes() == pk.tobytes()
    assert tuple(pk[1, 4]) == (0, 0) and tuple(pk[2, 1]) == (0, 0) and pk.max() > 0
    for s in range(ns):
        if nch[s] == 1:
            assert not pcm[:, s, 1].any(), s                         # a mono stream's second plane is zero fill
    b.close()


def _inter(streams, T, seed):
    ns = len(streams)
    x = np.stack([np.stack([gen_pcm(seed + s, (0, 7, 5, 4)[s % 4], 0, T)[f].T.reshape(-1) for s in range(ns)]) for f in range(T)])      # [T, ns, 2304] L R L R
    for s, (_, m, _, _) in enumerate(streams):
        if m == "m":
            x[:, s, I.FRAMES:] = 0x1234                              # a mono stream is its first 1152 values; the rest is never read
    return x


def _short_pattern(T, ns, seed):
    rng = np.random.default_rng(seed)
    fx = I.fixture()[0]
    v = np.where(rng.random((T, ns)) < 0.35, rng.choice(fx, size=(T, ns)), 1152).astype(np.int32)
    v[:, 0] = 1152
    return v


@pytest.mark.parametrize("egress,ngroups", [("frames", 2), ("af", 3)])
def test_tick_with_short_reads_equals_tick_fed_the_stretched_pcm(M, egress, ngroups):
    """some tens of ticks with a random short pattern (junk behind `valid`) against a second tick object that gets the stretched PCM,
    computed in numpy, as full reads: frames, packets and peaks of every stream are byte-equal; the counters follow the plain loop"""
    streams = [s for s in MIX if s[0] in (48000, 24000, 16000)] if egress == "af" else MIX
    cfgs, nch, ns, T = _cfgs(M, streams), _nch(streams), len(streams), 30
    rates = [r for r, _, _, _ in streams]
    inter = _inter(streams, T, 7300)
    valid = _short_pattern(T, ns, 17)
    assert (valid < 1152).sum() > 40
    stretched = I.stretch_batch(inter, valid, nch)
    junk = inter.copy()
    for f in range(T):
        for s in range(ns):
            v = int(valid[f, s])
            junk[f, s, (2 * v if nch[s] == 2 else v):(2304 if nch[s] == 2 else 1152)] = 0x6b6b
    kw = dict(egress=egress, ngroups=ngroups, version=b"short", now_s=1712345678, delay_ms=370, tist=True)
    a, b = M.Tick(cfgs, **kw), M.Tick(cfgs, **kw)
    a.enable_short_reads()
    for s in range(ns):
        a.set_gain_db(GAINS[s], s); b.set_gain_db(GAINS[s], s)
    snap = lambda t: [(t.frame(s), t.packets(s), tuple(int(x) for x in t.peaks[s]), int(t.silence_ms[s])) for s in range(ns)]
    ms, n = [0] * ns, [0] * ns
    for f in range(T + 1):
        if f < T:
            a.pcm[:] = junk[f]
            a.valid[:] = valid[f]
            b.pcm[:] = stretched[f]
            a.run(); b.run()
            ms, n = I.underrun_python(valid[f:f + 1], rates, ms, n)
            assert list(a.underrun_ms) == ms and list(a.underruns) == n, f
        else:
            a.finish(); b.finish()
            assert list(a.underrun_ms) == ms and list(a.underruns) == n
        got, want = snap(a), snap(b)
        for s in range(ns):
            assert got[s] == want[s], (f, s)
        if f >= 1:
            assert all(len(x[0]) > 0 or len(x[1]) > 0 for x in got)
    assert b.valid is None and b.underrun_ms is None and b.underruns is None
    a.close(); b.close()


def test_valid_array_alternates_with_the_input_sets(M):
    """tlb_tick_valid follows tlb_tick_pcm: NULL while two ticks are in flight; a set the caller does not touch reads as full when it is
    handed back; enabling after the first submit is refused"""
    streams = [(48000, "s", 128, 1)] * 5 + [(48000, "m", 64, 1)]
    cfgs, ns, T = _cfgs(M, streams), 6, 8
    inter = _inter(streams, T, 8100)
    t = M.Tick(cfgs, egress="frames", ngroups=2)
    assert t.valid is None and t.underrun_ms is None
    t.enable_short_reads()
    t.enable_short_reads()                                           # (again: no error, no change)
    assert list(t.valid) == [1152] * ns
    t.pcm[:] = inter[0]; t.valid[2] = 1100; p0 = t.valid.ctypes.data
    t.submit()
    p1 = t.valid.ctypes.data
    assert p1 != p0 and list(t.valid) == [1152] * ns
    t.pcm[:] = inter[1]; t.valid[3] = 1140
    t.submit()
    assert t.pcm is None and t.valid is None                         # two ticks in flight
    with pytest.raises(M.ToolameError) as e:
        t.enable_short_reads()
    assert e.value.code == 18
    t.wait()
    assert t.valid.ctypes.data == p0 and list(t.valid) == [1152] * ns          # the set of tick 0 again: stream 2's 1100 is gone
    assert list(t.underruns) == [0, 0, 1, 0, 0, 0] and list(t.underrun_ms) == [0, 0, 24, 0, 0, 0]
    t.pcm[:] = inter[2]                                              # untouched: every stream a full read
    t.submit()
    t.wait()
    assert list(t.underruns) == [0, 0, 1, 1, 0, 0] and list(t.underrun_ms) == [0, 0, 0, 24, 0, 0]
    t.wait()
    assert list(t.underruns) == [0, 0, 1, 1, 0, 0] and list(t.underrun_ms) == [0, 0, 0, 0, 0, 0]
    for f in range(3, T):                                            # run(): submit + wait, the sets still alternate and come back full
        t.pcm[:] = inter[f]
        assert list(t.valid) == [1152] * ns
        t.valid[5] = 1151
        t.run()
        assert t.underruns[5] == f - 2 and t.underrun_ms[5] == 24 * (f - 2)
    t.finish()
    assert t.valid is None
    # a fresh object: enabling is refused once a tick has been submitted
    u = M.Tick(cfgs, egress="frames")
    u.pcm[:] = inter[0]
    u.run()
    with pytest.raises(M.ToolameError) as e:
        u.enable_short_reads()
    assert e.value.code == 18 and u.valid is None and u.underrun_ms is None and u.underruns is None
    t.close(); u.close()


def test_node_accessors_land_in_the_right_shard(M):
    """devices = (0, 0, 0): a stream of shard 1 that is short on some ticks -- its own output equals a tick object fed the stretched PCM,
    its counters come back under its node-wide index, and shards 0 and 2 are byte-equal to an undisturbed node"""
    streams = (MIX + MIX)[:13]
    cfgs, nch, ns, T = _cfgs(M, streams), _nch(streams), 13, 12
    inter = _inter(streams, T, 9100)
    blocks = M.node_partition(ns, 3)
    victim = blocks[1][0] + 1
    assert blocks[1][0] <= victim < blocks[1][0] + blocks[1][1]
    valid = np.full((T, ns), 1152, np.int32)
    valid[[2, 3, 7, 10], victim] = [1100, 1151, 900, 1037]
    rate = streams[victim][0]
    stretched = I.stretch_batch(inter, valid, nch)
    snap = lambda nd: [(nd.frame(s), nd.peaks(s), nd.silence_ms(s)) for s in range(ns)]
    plain = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames")
    assert plain.valid(0) is None and plain.underruns(victim) == 0
    short = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames")
    short.enable_short_reads()
    ref = M.Node(cfgs, devices=(0, 0, 0), plane="tick", egress="frames")      # the victim's stretched PCM as full reads
    ms = n = 0
    for f in range(T):
        plain.set_pcm(inter[f]); short.set_pcm(inter[f]); ref.set_pcm(stretched[f])
        assert all(int(short.valid(s)[0]) == 1152 for s in range(ns))
        short.valid(victim)[0] = valid[f, victim]
        plain.run(); short.run(); ref.run()
        if valid[f, victim] < 1152:
            ms += I.frame_ms(rate); n += 1
        else:
            ms = 0
        a, b, c = snap(plain), snap(short), snap(ref)
        for s in range(ns):
            assert b[s] == c[s], (f, s)
            if s != victim:
                assert b[s] == a[s], (f, s)
            assert (short.underrun_ms(s), short.underruns(s)) == ((ms, n) if s == victim else (0, 0)), (f, s)
    with pytest.raises(M.ToolameError) as e:
        plain.enable_short_reads()                                   # after the first submit
    assert e.value.code == 18
    assert n == 4 and [x[0] for x in snap(plain)] != [x[0] for x in snap(short)]
    plain.close(); short.close(); ref.close()


def test_tick_never_enabled_is_what_it_was(M):
    """a tick object that never enables short reads: frames and peaks equal the stage-by-stage path (tlb_ingest_host without an array,
    tlb_encode_host_len), its three accessors return None"""
    streams = MIX[:7]
    cfgs, ns, T = _cfgs(M, streams), 7, 6
    inter = _inter(streams, T, 9900)
    b = M.Batch(cfgs)
    for s in range(ns):
        b.set_gain_db(GAINS[s], s)
    pcm, peaks = b.ingest(inter)
    lens = np.zeros((T, ns), dtype=np.int32)
    frames = np.zeros((T, ns, b.out_stride), dtype=np.uint8)
    assert b.L.tlb_encode_host_len(b.h, pcm.ctypes.data, T, None, None, frames.ctypes.data, lens.ctypes.data, None) == 0
    t = M.Tick(cfgs, egress="frames", ngroups=2)
    for s in range(ns):
        t.set_gain_db(GAINS[s], s)
    for f in range(T):
        t.pcm[:] = inter[f]
        assert t.valid is None and t.underrun_ms is None and t.underruns is None
        t.run()
        assert np.array_equal(t.peaks, peaks[f])
        for s in range(ns):
            assert t.frame(s) == frames[f, s, :lens[f, s]].tobytes(), (f, s)
    t.close(); b.close()
