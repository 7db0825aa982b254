"""The device resampler on the GPU (csrc/toolame_resample.hip, tlb_resample_*, tlb_tick_set_source, tlb_node_set_source): the device against
the oracle of tests/resamplelib.py byte for byte, the life-cycle calls, tick and node objects with sources against objects without that are
fed the oracle's resampled PCM, the exclusion of short reads, and one compare-monitor case."""
import numpy as np
import pytest

import resamplelib as R
from pcmgen import gen_pcm

pytestmark = pytest.mark.gpu
S = R.STREAMS
NS = len(S)


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def noise():
    sigs = R.signals(S, "noise")
    slots = R.cut(sigs, S, 0, R.NFRAMES)
    return sigs, slots, R.Oracle(S).resample(slots)


def _sourced(obj):
    for s, c in enumerate(S):
        if c["source"]:
            obj.set_source(c["source"], s)
    return obj


@pytest.mark.parametrize("cuts", [(6,), (1, 3, 2)])
def test_device_equals_oracle(M, noise, cuts):
    sigs, _, want = noise
    b = _sourced(M.Batch(R.stream_configs(S)))
    assert [b.source(s) for s in range(NS)] == [c["source"] for c in S]
    outs, f0 = [], 0
    for n in cuts:
        for s, c in enumerate(S):
            assert [b.need(s, k) for k in range(n)] == [R.need(c["source"], c["samplerate"], f0 + k) for k in range(n)], (f0, s)
        outs.append(b.resample(R.cut(sigs, S, f0, n, fill=0x7FFF)))
        f0 += n
    got = np.concatenate(outs)
    R.same(got, want, S, cuts)
    assert np.array_equal(got[:, 4], R.cut(sigs, S, 0, R.NFRAMES, fill=0x7FFF)[:, 4])
    assert (got[:, 1, R.N:] == 0).all()                              # behind a one-channel stream's 1152 values nothing is written
    b.close()


def test_life_cycle(M, noise):
    sigs, slots, want = noise
    b, o = _sourced(M.Batch(R.stream_configs(S))), R.Oracle(S)
    L = b.L
    R.same(b.resample(slots[:2]), o.resample(slots[:2]), S)
    b.stream_reset(0); o.reset(0)                                    # stream 0 starts again
    b.stream_finish(1); o.reset(1)                                   # ... stream 1 too
    b.stream_reconfigure(2, M.StreamConfig(samplerate=24000, mode="m", bitrate=32, psy_model=1)); o.reset(2)      # a legal one: 22.05 kHz still pairs with 24 kHz
    with pytest.raises(M.ToolameError) as e:
        b.stream_reconfigure(3, M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1))             # 16 kHz does not pair with 48 kHz
    assert e.value.code == 1 and b.source(3) == 16000 and b.source(2) == 22050
    b.set_source(16000, 3); o.reset(3)                               # set again between calls: fresh state
    assert L.tlb_resample_set_source(b.h, 0, 32000 + 1) == 1 and L.tlb_resample_set_source(b.h, -1, 44100) == 1 and b.source(0) == 44100
    assert [b.need(s) for s in range(4)] == [R.need(c["source"], c["samplerate"], 0) for c in S[:4]]
    nxt = R.cut(sigs, S, 0, 2)
    nxt[:, 4] = slots[2:4, 4]
    got = b.resample(nxt)
    R.same(got, o.resample(nxt), S)
    R.same(got[:, :4], want[:2, :4], S[:4])                          # frames 0 and 1 of fresh streams
    b.set_source(0, 0)                                               # off: the slot passes
    assert b.source(0) == 0 and b.need(0) == 1152
    assert np.array_equal(b.resample(slots[:1])[0, 0], slots[0, 0])
    d = np.zeros(2304 * NS + 8, dtype=np.int16)                      # host arrays standing in for device pointers: refused before any launch
    assert L.tlb_resample_device(b.h, d.ctypes.data, 1, d.ctypes.data, None) == 18
    b.reset()
    assert [b.need(s) for s in range(1, 4)] == [768, R.need(22050, 24000, 0), 768]
    b.close()


@pytest.mark.parametrize("egress", ["frames", "af"])
def test_tick_with_sources_equals_tick_fed_the_oracle_s_pcm(M, noise, egress):
    sigs, slots, want = noise
    kw = dict(egress=egress, ngroups=2, version=b"rs", now_s=1712345678, delay_ms=370, tist=True)
    a, b = M.Tick(R.stream_configs(S), **kw), M.Tick(R.stream_configs(S), **kw)
    _sourced(a)
    snap = lambda t: [(t.frame(s), t.packets(s), tuple(int(x) for x in t.peaks[s])) for s in range(NS)]
    for f in range(R.NFRAMES + 1):
        if f < R.NFRAMES:
            assert [a.need(s) for s in range(NS)] == [M.resample_need_at(c["source"], c["samplerate"], f) if c["source"] else 1152 for c in S], f
            assert [b.need(s) for s in range(NS)] == [1152] * NS
            a.pcm[:] = R.cut(sigs, S, f, 1, fill=0x7FFF)[0]
            b.pcm[:] = want[f]
            a.run(); b.run()
        else:
            a.finish(); b.finish()
        got, exp = snap(a), snap(b)
        for s in range(NS):
            assert got[s] == exp[s], (f, s)
        if f >= 1:
            assert all(len(x[0]) > 0 or len(x[1]) > 0 for x in got)
    a.close(); b.close()


def test_tick_without_a_source_is_what_it_was(M, noise):
    """no source set: the tick's frames and peaks equal the stage-by-stage path on the same input (ingest, encode), need is 1152.  This
    checks what such an object computes; which device calls it queues is not asserted (the submit's branch on `resample` is the statement).
    A source set and turned off again leaves the same object."""
    _, _, want = noise
    cfgs = R.stream_configs(S)
    b = M.Batch(cfgs)
    pcm, peaks = b.ingest(want)
    lens = np.zeros((R.NFRAMES, NS), dtype=np.int32)
    frames = np.zeros((R.NFRAMES, NS, b.out_stride), dtype=np.uint8)
    assert b.L.tlb_encode_host_len(b.h, pcm.ctypes.data, R.NFRAMES, None, None, frames.ctypes.data, lens.ctypes.data, None) == 0
    t = M.Tick(cfgs, egress="frames", ngroups=2)
    t.set_source(0)                                                  # "off" on an object that never had one: nothing happens
    t.set_source(44100, 0); t.set_source(0, 0)                       # on and off again: no source is set
    t.enable_short_reads()                                           # ... so short reads are not refused
    for f in range(R.NFRAMES):
        assert [t.need(s) for s in range(NS)] == [1152] * NS
        t.pcm[:] = want[f]
        t.run()
        assert np.array_equal(t.peaks, peaks[f])
        for s in range(NS):
            assert t.frame(s) == frames[f, s, :lens[f, s]].tobytes(), (f, s)
    t.close(); b.close()


def test_short_reads_and_a_source_exclude_each_other(M):
    cfgs = R.stream_configs(S)
    t = M.Tick(cfgs, egress="frames")
    t.enable_short_reads()
    with pytest.raises(M.ToolameError) as e:
        t.set_source(44100, 0)
    assert e.value.code == 18 and t.need(0) == 1152
    u = M.Tick(cfgs, egress="frames")
    u.set_source(44100, 0)
    with pytest.raises(M.ToolameError) as e:
        u.enable_short_reads()
    assert e.value.code == 18 and u.valid is None and u.need(0) == 1058
    with pytest.raises(M.ToolameError) as e:
        u.set_source(32000, 2)                                       # 32 kHz does not pair with 24 kHz
    assert e.value.code == 1
    nd = M.Node(cfgs, devices=(0, 0), plane="tick", egress="frames")
    nd.enable_short_reads()
    with pytest.raises(M.ToolameError) as e:
        nd.set_source(44100, 0)
    assert e.value.code == 18
    n2 = M.Node(cfgs, devices=(0, 0), plane="tick", egress="frames")
    n2.set_source(44100, 0)
    with pytest.raises(M.ToolameError) as e:
        n2.enable_short_reads()
    assert e.value.code == 18
    nb = M.Node(cfgs, devices=(0, 0), plane="batch")
    assert nb.L.tlb_node_need(nb.h, 0) == -18
    t.close(); u.close(); nd.close(); n2.close(); nb.close()


@pytest.mark.parametrize("egress", ["frames", "af"])
def test_node_with_sources_and_a_shard_restart(M, noise, egress):
    sigs, slots, want = noise
    cfgs = R.stream_configs(S)
    kw = dict(egress=egress, version=b"rs", now_s=1712345678, tist=True)
    nd = M.Node(cfgs, devices=(0, 0), plane="tick", **kw)
    for s, c in enumerate(S):
        if c["source"]:
            nd.set_source(c["source"], s)
    t = M.Tick(cfgs, **kw)
    blocks = M.node_partition(NS, 2)
    for f in range(4):
        assert [nd.need(s) for s in range(NS)] == [R.need(c["source"], c["samplerate"], f) for c in S], f
        nd.set_pcm(R.cut(sigs, S, f, 1)[0]); t.pcm[:] = want[f]
        nd.run(); t.run()
        for s in range(NS):
            assert nd.frame(s) == t.frame(s) and tuple(nd.peaks(s)) == tuple(t.peaks[s]), (f, s)
            assert nd.packets(s) == t.packets(s), (f, s)
    nd.shard_restart(0)                                              # block 0 starts again at need(0), block 1 goes on
    first, n0 = blocks[0]
    fresh = M.Tick(cfgs[first:first + n0], **kw)
    for k in range(2):
        for s in range(NS):
            in0 = first <= s < first + n0
            assert nd.need(s) == R.need(S[s]["source"], S[s]["samplerate"], k if in0 else 4 + k), (k, s)
        row = R.cut(sigs, S, 4 + k, 1)[0]
        row[first:first + n0] = R.cut(sigs, S, k, 1)[0][first:first + n0]
        nd.set_pcm(row); t.pcm[:] = want[4 + k]; fresh.pcm[:] = want[k, first:first + n0]
        nd.run(); t.run(); fresh.run()
        for s in range(NS):
            in0 = first <= s < first + n0
            assert nd.frame(s) == (fresh.frame(s - first) if in0 else t.frame(s)), (k, s)
            assert nd.packets(s) == (fresh.packets(s - first) if in0 else t.packets(s)), (k, s)      # (the restarted block's EDI senders start again, as a fresh object's)
    nd.close(); t.close(); fresh.close()


def test_compare_monitor_on_a_resampled_stream(M):
    """a 44.1 kHz source under the compare monitor with the default parameters: what is set against the decoded audio is the ingest's
    output at the encoder's rate, so every frame with a whole history is judged and none mismatches"""
    cfg = dict(samplerate=48000, mode="s", source=44100)
    T = 8
    total = R.total_need(cfg, T)
    sig = gen_pcm(seed=77, kind=0, frame=0, nframes=(total + R.N - 1) // R.N).transpose(1, 0, 2).reshape(2, -1)[:, :total].T.astype(np.int16)
    t = M.Tick(R.stream_configs([cfg], kbps=192), egress="frames")
    t.set_source(44100)
    t.enable_monitor("audio")
    t.enable_compare()
    for f in range(T):
        t.pcm[:] = R.cut([sig], [cfg], f, 1)[0]
        t.run()
    t.finish()
    rec = t.compare[0]
    print("compared %d judged %d mismatch %d" % (rec["frames_compared"], rec["frames_judged"], rec["mismatch_frames"]))
    assert rec["frames_compared"] == T and rec["frames_judged"] == T and rec["mismatch_frames"] == 0
    t.close()
