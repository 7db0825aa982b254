"""The device decimator on the GPU (csrc/toolame_decimate.hip, tlb_decimate_*, tlb_tick_set_down_source, tlb_node_set_down_source): the device
against the oracle of tests/decimatelib.py and the emulation byte for byte, the life-cycle calls, the buffer checks, tick and node objects with
down sources against objects without that are fed the oracle's decimated PCM, and the exclusion of sources, feeds and short reads."""
import numpy as np
import pytest

import decimatelib as D

pytestmark = pytest.mark.gpu
S = D.STREAMS
NS = len(S)
DOWN = [s for s, c in enumerate(S) if c["source"]]


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def noise():
    """the sources, the background of the output buffer (for streams 4 and 5: their own 24 / 48 kHz PCM) and the oracle's output on it"""
    sigs = D.signals(S, "noise")
    bg = D.background(D.NFRAMES, NS)
    return sigs, bg, D.Oracle(S).decimate(D.cut(sigs, S, 0, D.NFRAMES), bg)


def _down(obj, cfgs=S):
    for s, c in enumerate(cfgs):
        if c["source"]:
            obj.set_down_source(c["source"], s)
    return obj


@pytest.mark.parametrize("cuts", [(6,), (1, 3, 2)])
def test_device_equals_oracle_equals_emulation(M, noise, cuts):
    sigs, bg, want = noise
    b = _down(M.Batch(D.stream_configs(S)))
    assert [b.down_source(s) for s in range(NS)] == [c["source"] for c in S]
    emu = D.run_cuts(D.DecimateEmu(S).decimate, sigs, S, cuts, fill=0x7FFF, bg=bg)
    outs, f0 = [], 0
    for n in cuts:
        for s, c in enumerate(S):                                    # need follows the oracle across the cuts
            assert [b.down_need(s, k) for k in range(n)] == [D.need(c["source"], c["samplerate"], f0 + k) for k in range(n)], (f0, s)
        outs.append(b.decimate(D.cut(sigs, S, f0, n, fill=0x7FFF), bg[f0:f0 + n].copy()))
        f0 += n
    got = np.concatenate(outs)
    assert np.array_equal(got, want), (cuts, np.argwhere(got != want)[:4].tolist())
    assert np.array_equal(got, emu)
    assert np.array_equal(got[:, 4:], bg[:, 4:]) and np.array_equal(got[:, 1, D.N:], bg[:, 1, D.N:])      # left alone
    b.close()


def test_life_cycle(M, noise):
    sigs, bg, want = noise
    b, o = _down(M.Batch(D.stream_configs(S))), D.Oracle(S)
    L = b.L
    wide = D.cut(sigs, S, 0, D.NFRAMES)
    assert np.array_equal(b.decimate(wide[:2]), o.decimate(wide[:2]))
    assert [b.down_need(2, k) for k in range(4)] == [2117, 2117, 2116, 2117]      # two frames done: frames 2, 3, 4 and 5 = 0 of the cycle
    b.stream_reset(0); o.reset(0)                                    # stream 0 starts again
    b.stream_finish(1); o.reset(1)                                   # ... stream 1 too
    b.stream_reconfigure(2, M.StreamConfig(samplerate=24000, mode="s", bitrate=48, psy_model=1)); o.reset(2)      # a legal one: 44.1 kHz still pairs with 24 kHz
    with pytest.raises(M.ToolameError) as e:
        b.stream_reconfigure(3, M.StreamConfig(samplerate=48000, mode="m", bitrate=64, psy_model=1))              # 32 kHz is no down source of a 48 kHz stream
    assert e.value.code == 1 and b.down_source(3) == 32000 and b.down_source(2) == 44100
    b.set_down_source(32000, 3); o.reset(3)                          # set again between calls: fresh state
    # illegal rates, nothing changed: 48001; 44.1 kHz for every stream (stream 5 runs at 48 kHz: that pair is the resampler's); 32 kHz on stream 5
    assert L.tlb_decimate_set_source(b.h, 0, 48001) == 1 and L.tlb_decimate_set_source(b.h, -1, 44100) == 1 and L.tlb_decimate_set_source(b.h, 5, 32000) == 1
    assert [b.down_source(s) for s in range(NS)] == [c["source"] for c in S]
    assert [b.down_need(s) for s in range(NS)] == [D.need(c["source"], c["samplerate"], 0) for c in S]
    got = b.decimate(wide[:2])
    assert np.array_equal(got, o.decimate(wide[:2]))
    for s in DOWN:
        n = D.nch_of(S[s]) * D.N
        assert np.array_equal(got[:, s, :n], want[:2, s, :n])        # frames 0 and 1 of fresh streams
    b.set_down_source(0, 0)                                          # off: the slot is left alone
    assert b.down_source(0) == 0 and b.down_need(0) == 1152
    assert np.array_equal(b.decimate(wide[:1], bg[:1].copy())[0, 0], bg[0, 0])
    b.set_source(22050, 4)                                           # an up source on stream 4: a down source on it is refused, and nothing changes
    assert L.tlb_decimate_set_source(b.h, 4, 48000) == 18 and b.down_source(4) == 0
    b.reset()
    assert [b.down_need(s) for s in (1, 2, 3)] == [2304, 2117, 1536]
    b.close()


def test_up_source_on_a_stream_with_a_down_source_is_refused(M):
    """the other direction of test_life_cycle's last refusal, setters only: a stream has one source whichever family comes first"""
    b = M.Batch(D.stream_configs(S))
    b.set_down_source(48000, 0)                                      # stream 0 runs at 24 kHz: 16 kHz would be a legal up source of it
    assert b.L.tlb_resample_set_source(b.h, 0, 16000) == 18
    assert b.source(0) == 0 and b.down_source(0) == 48000
    b.close()


def test_overlapping_and_misaligned_buffers_are_refused(M):
    """host arrays standing in for device pointers: refused before any launch"""
    b = _down(M.Batch(D.stream_configs(S)))
    L = b.L
    d = np.zeros(D.WIDE * NS * 2 + 64, dtype=np.int16)
    base = d.ctypes.data + (-d.ctypes.data) % 16
    out = base + D.WIDE * NS * 2                                     # right behind one frame of wide slots: legal as far as the checks go
    assert L.tlb_decimate_device(b.h, base, 1, base, None) == 18
    assert L.tlb_decimate_device(b.h, base, 1, base + D.WIDE * NS * 2 - 16, None) == 18      # the output begins inside the wide buffer
    assert L.tlb_decimate_device(b.h, base + 2304 * NS * 2 - 16, 1, base, None) == 18        # the wide buffer begins inside the output
    assert L.tlb_decimate_device(b.h, base + 2, 1, out, None) == 18 and L.tlb_decimate_device(b.h, base, 1, out + 8, None) == 18
    assert L.tlb_decimate_device(b.h, base, 0, out, None) == 18
    assert [b.down_need(s) for s in range(4)] == [2304, 2304, 2117, 1536]      # no call advanced a position
    b.close()


def _snap(t, n):
    return [(t.frame(s), tuple(int(x) for x in t.peaks[s])) for s in range(n)]


def _tick_pair(M, cfgs, sigs, pcm24, nframes):
    """a Tick with down sources on the wide slots against a Tick without on pcm24, tick by tick, two ticks overlapped via submit / wait"""
    ns = len(cfgs)
    kw = dict(egress="frames", ngroups=2)
    a, b = _down(M.Tick(D.stream_configs(cfgs), **kw), cfgs), M.Tick(D.stream_configs(cfgs), **kw)
    down = [s for s, c in enumerate(cfgs) if c["source"]]

    def fill(f):
        assert [a.down_need(s) for s in range(ns)] == [D.need(c["source"], c["samplerate"], f) for c in cfgs], f
        wide = D.cut(sigs, cfgs, f, 1, fill=0x7FFF)[0]
        pa = a.pcm
        pa[:] = pcm24[f]
        for s in down:
            pa[s] = 0x7FFF                                           # the PCM slot of a down stream is the decimator's to write
            a.down(s)[:] = wide[s]
        b.pcm[:] = pcm24[f]

    assert b.down(0) is None and b.down_need(0) == 1152
    fill(0); a.submit(); b.submit()
    for f in range(1, nframes + 1):
        if f < nframes:
            fill(f); a.submit(); b.submit()
            assert a.down(down[0]) is None and a.pcm is None         # two ticks in flight
        a.wait(); b.wait()
        assert _snap(a, ns) == _snap(b, ns), f
        if f >= 2:
            assert all(len(x[0]) > 0 for x in _snap(a, ns))
    a.finish(); b.finish()
    assert _snap(a, ns) == _snap(b, ns)
    a.close(); b.close()


def test_tick_with_down_sources_equals_tick_fed_the_oracle_s_pcm(M, noise):
    sigs, bg, want = noise                                           # groups {0, 1, 2} (all down) and {3, 4, 5} (mixed)
    _tick_pair(M, S, sigs, want, D.NFRAMES)


def test_tick_whose_every_stream_has_a_down_source(M, noise):
    sigs, bg, want = noise                                           # no group's PCM is copied in
    _tick_pair(M, S[:4], sigs[:4], want[:, :4], D.NFRAMES)


def test_node_with_down_sources_and_a_shard_restart(M, noise):
    sigs, bg, want = noise
    cfgs = D.stream_configs(S)
    nd = _down(M.Node(cfgs, devices=(0, 0), plane="tick", egress="frames"))
    t = M.Tick(cfgs, egress="frames")
    blocks = M.node_partition(NS, 2)

    def fill(row_of):
        pcm = np.stack([want[row_of(s), s] for s in range(NS)])
        nd.set_pcm(pcm)
        for s in DOWN:
            nd.down(s)[:] = D.cut(sigs, S, row_of(s), 1, fill=0x7FFF)[0, s]

    for f in range(3):
        assert [nd.down_need(s) for s in range(NS)] == [D.need(c["source"], c["samplerate"], f) for c in S], f
        fill(lambda s: f); t.pcm[:] = want[f]
        nd.run(); t.run()
        for s in range(NS):
            assert nd.frame(s) == t.frame(s) and tuple(nd.peaks(s)) == tuple(t.peaks[s]), (f, s)
    nd.shard_restart(0)                                              # block 0 starts again at need(0) with its down sources, block 1 goes on
    first, n0 = blocks[0]
    fresh = M.Tick(cfgs[first:first + n0], egress="frames")
    for k in range(2):
        in0 = lambda s: first <= s < first + n0
        for s in range(NS):
            assert nd.down_need(s) == D.need(S[s]["source"], S[s]["samplerate"], k if in0(s) else 3 + k), (k, s)
        fill(lambda s: k if in0(s) else 3 + k); t.pcm[:] = want[3 + k]; fresh.pcm[:] = want[k, first:first + n0]
        nd.run(); t.run(); fresh.run()
        for s in range(NS):
            assert nd.frame(s) == (fresh.frame(s - first) if in0(s) else t.frame(s)), (k, s)
    nb = M.Node(cfgs, devices=(0, 0), plane="batch")
    assert nb.L.tlb_node_down_need(nb.h, 0) == -18 and nb.down(0) is None
    nd.close(); t.close(); fresh.close(); nb.close()


def test_down_sources_sources_feeds_and_short_reads_exclude_one_another(M):
    cfgs = D.stream_configs(S)
    feed = M.FeedConfig(samplerate=24000, bitrate=64, channels=2)
    others = {"source": lambda o: o.set_source(22050, 4), "feed": lambda o: o.set_feed(4, feed), "short reads": lambda o: o.enable_short_reads()}
    for make in (lambda: M.Tick(cfgs, egress="frames"), lambda: M.Node(cfgs, devices=(0, 0), plane="tick", egress="frames")):
        for name, other in others.items():
            x = make()                                               # the other one first: a down source is refused
            other(x)
            with pytest.raises(M.ToolameError) as e:
                x.set_down_source(48000, 0)
            assert e.value.code == 18 and x.down_need(0) == 1152 and x.down(0) is None, name
            x.close()
            y = make()                                               # a down source first: the other one is refused
            y.set_down_source(48000, 0)
            with pytest.raises(M.ToolameError) as e:
                other(y)
            assert e.value.code == 18 and y.down_need(0) == 2304, name
            y.close()
    t = M.Tick(cfgs, egress="frames")
    with pytest.raises(M.ToolameError) as e:
        t.set_down_source(32000, 5)                                  # 32 kHz is no down source of a 48 kHz stream
    assert e.value.code == 1
    t.set_down_source(0)                                             # "off" on an object that never had one: nothing happens
    t.set_down_source(48000, 0); t.set_down_source(0, 0)             # on and off again: no down source is set
    assert t.down(0) is None and t.down_need(0) == 1152
    t.enable_short_reads()                                           # ... so short reads are not refused
    t.close()
