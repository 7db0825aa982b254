"""Every legal Layer II configuration -- 6 sample rates x 4 modes x 14 bitrates = 336 (rate, mode, bitrate) triples, all five allocation
tables -- through the lane-loop emulation of the encoder (csrc/mp2_wave.h) and of the frame check / decoder (csrc/mp2_unpack.h,
csrc/mp2_synth.h), without a GPU: bytes and parsed fields against the oracle, an independent bit reader, the numpy statement of the
standard's synthesis, damage once per table, and the oracle against the live reference where the goldens had a hole (table B.2d, the
highest rates).  tests/sweeplib.py holds what this module shares with the device's sweep (test_config_sweep_gpu.py)."""
import shutil

import numpy as np
import pytest

import declib as D
import emulib as E
import oraclelib as O
import sweeplib as S
import test_decode_emu as TE

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
PSYS = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return D.build_emu(tmp_path_factory.mktemp("decemu"))


class Sweep:
    """one psy model's 336 streams: the oracle's bytes and taps, its frames, and what the emulated decoder makes of them as ONE mixed batch"""

    def __init__(self, emu_so, psy):
        self.triples = S.legal_configs()
        self.cfgs, self.pcm = S.sweep_streams(psy)
        self.data, self.taps = S.oracle_sweep(self.cfgs, self.pcm)
        self.frames = [D.cut_frames(d, c) for d, c in zip(self.data, self.cfgs)]
        assert all(len(f) == S.NFRAMES for f in self.frames)
        e = D.DecEmu(emu_so, self.cfgs)
        fr, ln = D.batch_arrays(self.frames, e.stride)
        self.rep, self.fl, _ = e.decode(fr, ln, True, False)
        self.bad = e.bad_frames()
        e.close()


@pytest.fixture(scope="module")
def sweeps(emu_so):
    cache = {}

    def get(psy):
        if psy not in cache:
            cache[psy] = Sweep(emu_so, psy)
        return cache[psy]
    return get


def test_legal_configurations_and_their_tables():
    """336 triples, found by trying; 60 / 48 / 40 / 20 / 168 of them on tables B.2a / B.2b / B.2c / B.2d / LSF (sweeplib.legal_configs
    asserts both, and that declib.pick_table names the table the oracle selected).  The named groups of this module are what the issue
    counted: 20 B.2d triples, 24 at 8 / 16 kbps LSF, 39 at 160 kbps per channel or more."""
    legal = S.legal_configs()
    assert len(legal) == len(set(legal)) == 336
    assert sum(S.table_of(t) == 3 for t in legal) == 20 and all(t[0] == 32000 and S.per_channel(t) <= 48 for t in legal if S.table_of(t) == 3)
    assert sum(map(S.is_low_table, legal)) == 60 and sum(map(S.is_lsf_floor, legal)) == 24 and sum(map(S.is_top_rate, legal)) == 39
    assert sum(S.per_channel(t) == 192 for t in legal) == 12       # 'm' 192 and 's' / 'j' / 'd' 384 at the three MPEG-1 rates


@pytest.mark.parametrize("psy", PSYS)
def test_emulated_encoder_equals_the_oracle_on_every_configuration(sweeps, psy):
    """all 336 triples as ONE batch of 6 frames, fed in ragged calls (the padding-slot recurrence of 44.1 / 22.05 kHz crosses them), a
    different signal per stream: byte for byte the oracle's stream"""
    w = sweeps(psy)
    b = E.EmuBatch(w.cfgs)
    got, pos = [b""] * len(w.cfgs), 0
    for n in (1, 3, 2):
        g, _ = b.encode(w.pcm[pos:pos + n])
        got = [a + c for a, c in zip(got, g)]
        pos += n
    assert pos == S.NFRAMES
    tail = b.flush()
    b.close()
    bad = [t for t, g, x, want in zip(w.triples, got, tail, w.data) if g + x != want]
    assert not bad, (psy, bad)
    # (frames of both lengths did occur, so the recurrence was exercised)
    assert any(len({len(f) for f in fr}) == 2 for fr, c in zip(w.frames, w.cfgs) if c["samplerate"] in (44100, 22050))


@pytest.mark.parametrize("psy", PSYS)
def test_emulated_decoder_fields_equal_the_oracles_taps(sweeps, psy):
    """the oracle's frames of the sweep, decoded as ONE mixed batch: every frame passes (only frame 0 is SCFCRC_UNCHECKED), and bit_alloc,
    scfsi, scalar and subband equal the oracle's taps exactly, under the masks of test_decode_emu.test_fields_equal_the_reference_taps"""
    w = sweeps(psy)
    assert w.bad == 0
    cells = 0
    for s, (t, cfg) in enumerate(zip(w.triples, w.cfgs)):
        nch = 1 if cfg["mode"] == "m" else 2
        for f in range(S.NFRAMES):
            r, tap = w.rep[f, s], w.taps[s][f]
            assert int(r["status"]) == (D.SCFCRC_UNCHECKED if f == 0 else 0), (psy, t, f, hex(int(r["status"])))
            assert (int(r["mode"]), int(r["mode_ext"])) == (tap["mode"], tap["mode_ext"]), (psy, t, f)
            assert int(r["crc_stored"]) == int(r["crc_computed"]), (psy, t, f)
            cells += S.assert_fields_equal_taps(w.fl[f, s], tap, nch, (psy, t, f))
    assert cells > 1_000_000


def test_sweep_reaches_every_requantiser_cell(sweeps):
    """Over the decoded sweep: all 87 (allocation-table line, allocation index) pairs, all five tables, both ScF-CRC layouts, the three
    grouped quantisers and the 65535-step class.  Each by name, so that a change of signals cannot silently lose one."""
    cells, tables, exts = set(), set(), set()
    for psy in PSYS:
        w = sweeps(psy)
        cells |= S.cells_of(w.cfgs, w.fl)
        for s, c in enumerate(w.cfgs):
            if w.fl["bit_alloc"][:, s].any():
                tables.add(D.pick_table(c)); exts.add(D.dab_ext_of(c))
    full = S.all_cells()
    assert len(full) == 87
    print(f"requantiser cells reached: {len(cells & full)}/{len(full)}")
    assert cells <= full, sorted(cells - full)
    for cell in sorted(full):
        assert cell in cells, ("(line, index) never decoded", cell)
    assert (4, 15) in cells                                        # the last one to be reached: needs the pure low tone on a B.2c / B.2d stream
    assert tables == {0, 1, 2, 3, 4}
    assert exts == {2, 4}
    steps, grouped = S.steps_of(cells)
    for n in (3, 5, 9):
        assert n in grouped, ("grouped quantiser never decoded", n)
    assert grouped == {3, 5, 9}
    assert 65535 in steps
    assert steps == set(D.RQ)                                     # every line of table 3-B.4


@pytest.mark.parametrize("psy", PSYS)
def test_independent_reader_agrees_on_the_sweep(sweeps, psy):
    """declib.read_frame (plain Python over np.unpackbits) on EVERY frame of the sweep (it costs seconds, so nothing is thinned) -- the
    60 B.2c / B.2d streams, the 24 at 8 / 16 kbps LSF and the 39 at 160 kbps per channel or more among them: CRC-16 computed == stored ==
    the device path's, audio_bits, the ScF-CRC against the tail of the frame before, and all four field arrays"""
    w = sweeps(psy)
    visits = [(s, f) for s in range(len(w.triples)) for f in range(S.NFRAMES)]
    named = [s for s, t in enumerate(w.triples) if S.is_low_table(t) or S.is_lsf_floor(t) or S.is_top_rate(t)]
    assert len(named) == 60 + 24 + 39 and all((s, f) in set(visits) for s in named for f in range(S.NFRAMES))
    for s, f in visits:
        t, cfg, fr = w.triples[s], w.cfgs[s], w.frames[s]
        info = D.read_frame(fr[f], cfg)
        r = w.rep[f, s]
        assert info["crc_computed"] == int(r["crc_computed"]) == info["crc_stored"] == int(r["crc_stored"]), (psy, t, f)
        assert info["audio_bits"] == int(r["audio_bits"]), (psy, t, f)
        assert (info["tab"], info["jsbound"]) == (D.pick_table(cfg), w.taps[s][f]["jsbound"]), (psy, t, f)
        if f > 0:
            assert info["scfcrc"] == D.stored_scfcrc(fr[f - 1], cfg), (psy, t, f)
        if f == S.NFRAMES - 1:
            assert info["scfcrc"] == D.stored_scfcrc(fr[f], cfg), (psy, t, f)          # the last frame carries its own
        for k in S.TAP_KEYS:
            assert np.array_equal(info[k], w.fl[f, s][k].astype(int)), (psy, t, f, k)


def test_pcm_equals_the_standards_flow_chart_on_the_sweep(emu_so):
    """The bound of test_decode_emu.test_pcm_equals_the_standards_flow_chart (two fp64 evaluations that differ in summation order only:
    |difference| <= 1 on at most 10 samples per million compared, audio and not silence) on every B.2c / B.2d triple, every triple at
    160 kbps per channel or more and 24 more that take in all six rates and all four modes; psy 1, signals that are not near-silence."""
    named, spread = S.pcm_triples()
    assert len(named) == 60 + 39 and len(spread) >= 24
    triples = named + spread
    cfgs, pcm = S.sweep_streams(1, triples=triples, signals=S.LOUD_SIGNALS)
    data, _ = S.oracle_sweep(cfgs, pcm)
    frames = [D.cut_frames(d, c) for d, c in zip(data, cfgs)]
    e = D.DecEmu(emu_so, cfgs)
    fr, ln = D.batch_arrays(frames, e.stride)
    rep, fl, got = e.decode(fr, ln, True, True)
    assert e.bad_frames() == 0 and not rep["status"][1:].any()
    e.close()
    total = flips = 0
    for s, (t, cfg) in enumerate(zip(triples, cfgs)):
        want = TE.numpy_pcm(frames[s], fl[:, s], cfg)
        d = np.abs(got[:, s].astype(np.int64) - want.astype(np.int64))
        assert d.max() <= 1, (t, int(d.max()))
        assert np.abs(want).max() > 1000, t                      # audio, not silence
        total += d.size
        flips += int((d != 0).sum())
    print(f"sweep decode PCM vs numpy: {flips} rounding flips in {total} samples of {len(triples)} streams")
    assert flips * 1_000_000 <= 10 * total, (flips, total)


# ---- damage, once per table ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def damage_set():
    return S.damage_streams()


def test_damage_is_found_and_contained_on_every_table(emu_so, damage_set):
    """test_decode_emu.run_damage (a header, allocation, scfsi, scalefactor and sync bit, a lost tail) and its truncation case on
    sweeplib.DAMAGE_CONFIGS: all five tables, both ScF-CRC layouts, 32000 'j' 96 (B.2d), 44100 'j' 96 and 48000 's' 384 among them"""
    fl, cfgs = damage_set
    assert len(cfgs) >= 8
    for t in ((32000, "j", 96), (44100, "j", 96), (48000, "s", 384)):
        assert t in [(c["samplerate"], c["mode"], c["kbps"]) for c in cfgs]
    TE.run_damage(lambda c: D.DecEmu(emu_so, c), fl, cfgs)
    TE.run_truncation(lambda c: D.DecEmu(emu_so, c), fl, cfgs)     # frame 5 of stream 2: 48000 's' 384


def test_sweep_damage_cases_are_clean_under_asan_ubsan(tmp_path, emu_so, damage_set):
    """the same inputs, with the padding-bit and noise batches of test_decode_emu.hostile_cases_of, through the AddressSanitizer + UBSan
    build of the lane-loop decoder: clean, and byte for byte the plain build's reports, fields and PCM"""
    fl, cfgs = damage_set
    exe = D.build_san_driver(tmp_path)
    e = D.DecEmu(emu_so, cfgs)
    cases = TE.hostile_cases_of(fl, cfgs, e.stride, S.DAMAGE_PAD_STREAM)
    got = D.run_san_driver(exe, tmp_path, cfgs, cases)
    assert len(got) == len(cases) >= 11
    for (fr, ln), g in zip(cases, got):
        e.reset()
        want = e.decode(fr, ln, True, True)
        for k in range(3):
            assert g[k].tobytes() == want[k].tobytes(), k
    e.close()


# ---- the oracle against the live reference, where the goldens had a hole ------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_oracle_equals_the_live_reference_on_b2d_and_the_top_rate():
    """the 20 B.2d triples and the four triples at 192 kbps per channel ('m' 192 at the three MPEG-1 rates is 3, 's' / 'j' / 'd' 384 nine
    more: all twelve are run), psy 1 and one other model each, 12 frames, taps on two of them: bytes, burst lengths and every tap"""
    if not O.REF_SO.exists():
        pytest.skip("oracle/_ref/libtoolame_ref.so not built here")
    legal = S.legal_configs()
    triples = [t for t in legal if S.table_of(t) == 3] + [t for t in legal if S.per_channel(t) == 192]
    assert len(triples) == 20 + 12
    nf, tap_frames, n = 12, (1, 7), 0
    for i, (fs, mode, kbps) in enumerate(triples):
        for psy in (1, (0, 2, 3, 4)[i % 4]):
            pcm = S.signal_pcm(i, S.LOUD_SIGNALS[(i + psy) % len(S.LOUD_SIGNALS)], nf, 9100 + 10 * i + psy)
            ref = O.reference_stream(pcm, samplerate=fs, mode=mode, kbps=kbps, psy=psy, tap_frames=tap_frames)
            assert ref["rc"] == [0] * 6, (fs, mode, kbps, psy, ref["rc"])
            e = O.OracleEncoder(samplerate=fs, mode=mode, kbps=kbps, psy=psy)
            nch, sbl = e.nch, e.sblimit
            chunks, lens = [], []
            for f in range(nf):
                chunks.append(e.encode(pcm[f])); lens.append(len(chunks[-1]))
                if f in tap_frames:
                    t, g, where = e.taps(), ref["taps"][f], (fs, mode, kbps, psy, f)
                    assert np.array_equal(t["scalar"][:nch, :, :sbl], g["scalar"][:nch, :, :sbl]), where
                    assert np.array_equal(t["scfsi"][:nch, :sbl], g["scfsi"][:nch, :sbl]), where
                    assert np.array_equal(t["bit_alloc"][:nch], g["bit_alloc"][:nch]), where
                    assert np.array_equal(t["subband"][:nch], g["subband"][:nch]), where
                    assert np.array_equal(_bits(t["sb_sample"][:nch]), _bits(g["sb_sample"][:nch])), where
                    assert np.array_equal(_bits(t["max_sc"][:nch]), _bits(g["max_sc"][:nch])), where
                    nsmr = sbl if psy == 1 else 32           # psy 1 writes only sblimit entries
                    assert np.array_equal(_bits(t["smr"][:nch, :nsmr]), _bits(g["smr"][:nch, :nsmr])), where
                    assert (t["mode"], t["mode_ext"]) == (g["mode"], g["mode_ext"]), where
                    if mode == "j":
                        assert np.array_equal(t["j_scale"][:, :sbl], g["j_scale"][:, :sbl]), where
            chunks.append(e.finish()); lens.append(len(chunks[-1]))
            e.close()
            assert b"".join(chunks) == ref["data"] and lens == list(ref["lens"]), (fs, mode, kbps, psy)
            n += 1
    assert n == 64

