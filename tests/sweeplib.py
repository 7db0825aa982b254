"""Support for the configuration sweeps (test_config_sweep_emu.py, test_config_sweep_gpu.py): every (sample rate, mode, bitrate) the
oracle accepts, found by trying; the signal of every stream of a sweep; the oracle's bytes and taps for it; and which (allocation-table
line, allocation index) cells a batch of parsed frames has been through.  A plain module: nothing here is collected by pytest."""
import numpy as np

import declib as D
import oraclelib as O
from pcmgen import gen_pcm

RATES = (48000, 44100, 32000, 24000, 22050, 16000)
MODES = "sjdm"
NCONFIGS = 336
TABLE_SPLIT = {0: 60, 1: 48, 2: 40, 3: 20, 4: 168}                # B.2a, B.2b, B.2c, B.2d, 13818-3 B.1
NFRAMES = 6
SIGNALS = (0, 2, 4, 5, 6, 7, "tone")                             # pcmgen kinds (no silence, no lone impulse: the reference's psy 3 crashes on them) + tone_pcm
LOUD_SIGNALS = (0, 2, 4, 5, 7, "tone")                           # ... without the +-1 LSB noise: what decodes to audio, not near-silence

_LEGAL = None


def legal_configs():
    """every (samplerate, mode, kbps) oraclelib.OracleEncoder accepts, in a fixed order.  Found by TRYING every multiple of 8 kbps up to
    448 (14 bitrates per MPEG-1 rate, 14 per LSF rate: 6 x 4 x 14 = 336), and split by allocation table as declib.pick_table (2.4.2.3)
    says, which has to agree with the table the oracle itself selected."""
    global _LEGAL
    if _LEGAL is None:
        out, split = [], {}
        L = O.lib()
        for fs in RATES:
            for mode in MODES:
                for kbps in range(8, 449, 8):
                    try:
                        e = O.OracleEncoder(samplerate=fs, mode=mode, kbps=kbps, psy=1)
                    except ValueError:
                        continue
                    tab = D.pick_table(dict(samplerate=fs, mode=mode, kbps=kbps))
                    assert L.mp2o_tablenum(e.h) == tab, (fs, mode, kbps, L.mp2o_tablenum(e.h), tab)
                    assert e.sblimit == int(D._tables()["sblimit"][tab]) and e.frame_bytes == D.frame_bytes_of(dict(samplerate=fs, kbps=kbps))
                    assert L.mp2o_dab_extension(e.h) == D.dab_ext_of(dict(samplerate=fs, mode=mode, kbps=kbps))
                    e.close()
                    split[tab] = split.get(tab, 0) + 1
                    out.append((fs, mode, kbps))
        assert len(out) == NCONFIGS, len(out)
        assert split == TABLE_SPLIT, split
        _LEGAL = out
    return list(_LEGAL)


def per_channel(triple):
    fs, mode, kbps = triple
    return kbps // (1 if mode == "m" else 2)


def table_of(triple):
    return D.pick_table(dict(samplerate=triple[0], mode=triple[1], kbps=triple[2]))


def tone_pcm(i, nframes):
    """a pure low tone, both channels equal: nearly every bit of the frame goes to subband 0, which is how the highest allocation
    indices of the low subbands' table lines are reached"""
    n = np.arange(nframes * 1152, dtype=np.float64)
    v = np.rint(30000.0 * np.sin(2.0 * np.pi * (40 + 3 * (i % 50)) * n / 48000.0)).astype(np.int16)
    return np.ascontiguousarray(np.broadcast_to(v.reshape(nframes, 1, 1152), (nframes, 2, 1152)))


def signal_pcm(i, which, nframes, seed):
    return tone_pcm(i, nframes) if which == "tone" else gen_pcm(seed, which, 0, nframes)


def sweep_streams(psy, nframes=NFRAMES, triples=None, signals=SIGNALS):
    """-> (cfgs, pcm [nframes][nstreams][2][1152]): one stream per triple, the signal turning with the stream index and the psy model.
    legal_configs() comes in blocks of 14 bitrates, twice the number of signals: the block number is added, so that a bitrate meets
    another signal in every (rate, mode) block instead of the same one throughout."""
    triples = legal_configs() if triples is None else list(triples)
    cfgs = [dict(samplerate=fs, mode=mode, kbps=kbps, psy=psy, pad_len=0) for fs, mode, kbps in triples]
    pcm = np.stack([signal_pcm(i, signals[(i + i // 14 + 3 * psy) % len(signals)], nframes, 7000 + 1000 * psy + i) for i in range(len(cfgs))], axis=1)
    return cfgs, pcm


TAP_KEYS = ("bit_alloc", "scfsi", "scalar", "subband")


def oracle_sweep(cfgs, pcm):
    """-> (per stream: all bytes, finish() included; per stream, per frame: the oracle's taps bit_alloc, scfsi, scalar, subband, jsbound,
    mode, mode_ext)"""
    data, taps = [], []
    for s, c in enumerate(cfgs):
        e = O.OracleEncoder(samplerate=c["samplerate"], mode=c["mode"], kbps=c["kbps"], psy=c["psy"], pad_len=c.get("pad_len", 0))
        chunks, tt = [], []
        for f in range(pcm.shape[0]):
            chunks.append(e.encode(pcm[f, s]))
            t = e.taps()
            tt.append({k: t[k] for k in TAP_KEYS + ("jsbound", "mode", "mode_ext")})
        chunks.append(e.finish())
        e.close()
        data.append(b"".join(chunks))
        taps.append(tt)
    return data, taps


def assert_fields_equal_taps(fields, taps, nch, where):
    """the masks of test_decode_emu.test_fields_equal_the_reference_taps: bit_alloc over every (channel, subband) of the stream; scfsi and
    scalar where the frame transmits them; subband where it transmits samples (an allocation, channel 1 below the bound only).  Returns
    the number of sample cells compared."""
    ba = fields["bit_alloc"].astype(int)
    assert np.array_equal(ba[:nch], taps["bit_alloc"][:nch]), (where, "bit_alloc")
    m = ba != 0
    assert not m[nch:].any(), where
    assert np.array_equal(fields["scfsi"][m], taps["scfsi"][m]), (where, "scfsi")
    m3 = np.broadcast_to(m[:, None, :], (2, 3, 32))
    assert np.array_equal(fields["scalar"][m3], taps["scalar"][m3]), (where, "scalar")
    own = m.copy()
    own[1, taps["jsbound"]:] = False
    ms = np.broadcast_to(own[:, None, None, :], (2, 3, 12, 32))
    assert np.array_equal(fields["subband"][ms].astype(np.int64), taps["subband"][ms].astype(np.int64)), (where, "subband")
    return int(ms.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage of the requantiser's cells, from the reference's own tables (tests/golden/tables_rates.npz)
def all_cells():
    """every (allocation-table line, allocation index >= 1) a legal frame can carry: the lines the five tables use below their sblimit,
    and 2^nbal - 1 indices each"""
    T = D._tables()
    lines = {int(T["line"][tab][sb]) for tab in range(5) for sb in range(int(T["sblimit"][tab]))}
    return {(ln, i) for ln in lines for i in range(1, 1 << int(T["nbal"][ln]))}


def cells_of(cfgs, fields):
    """fields [nframes][nstreams] as the decoder parsed them -> the (line, index) pairs present, and the step counts of their quantisers"""
    T = D._tables()
    cells = set()
    for s, c in enumerate(cfgs):
        tab, nch = D.pick_table(c), 1 if c["mode"] == "m" else 2
        sbl = int(T["sblimit"][tab])
        ba = fields["bit_alloc"][:, s, :nch, :sbl].astype(int)                    # [nframes][nch][sbl]
        for sb in range(sbl):
            ln = int(T["line"][tab][sb])
            cells |= {(ln, int(i)) for i in np.unique(ba[:, :, sb]) if i}
    return cells


def steps_of(cells):
    """the number of steps of each cell's quantiser, and which of them are grouped (three samples in one code)"""
    T = D._tables()
    q = [int(T["step_index"][ln][i]) for ln, i in cells]
    return {int(T["steps"][k]) for k in q}, {int(T["steps"][k]) for k in q if int(T["group"][k]) != 3}


# ---------------------------------------------------------------------------------------------------------------------------------
# the named groups of the sweep
def is_low_table(t):
    """B.2c or B.2d: at most 48 kbps per channel at an MPEG-1 rate"""
    return table_of(t) in (2, 3)


def is_top_rate(t):
    """160 kbps per channel or more: where the runs of 16-bit sample codes are"""
    return per_channel(t) >= 160


def is_lsf_floor(t):
    """8 or 16 kbps at a half rate: almost nothing is allocated"""
    return t[0] < 32000 and t[2] <= 16


def pcm_triples():
    """the triples whose decoded PCM is compared with the numpy statement: every B.2c / B.2d triple, every triple at 160 kbps per channel
    or more, and 24 of the others spread evenly over legal_configs()"""
    legal = legal_configs()
    named = [t for t in legal if is_low_table(t) or is_top_rate(t)]
    rest = [t for t in legal if t not in named]
    spread = [rest[i * len(rest) // 24] for i in range(24)]
    assert len(set(spread)) == 24 and {t[0] for t in spread} == set(RATES) and {t[1] for t in spread} == set(MODES)
    return named, spread


# the damage set: a stream per allocation table, the three layouts the goldens' damage set does not have among them -- B.2d
# (32000 'j' 96), a 2-byte-ScF-CRC B.2c stream with padding slots (44100 'j' 96), and the longest frame there is at 48 kHz (48000 's' 384)
DAMAGE_CONFIGS = [(32000, "j", 96, 3), (44100, "j", 96, 1), (48000, "s", 384, 1), (16000, "m", 8, 2), (44100, "s", 192, 0),
                  (32000, "m", 48, 1), (24000, "d", 160, 4), (48000, "m", 192, 2)]
DAMAGE_PAD_STREAM = 1                                            # frames of two lengths: the stream whose padding bit is flipped
DAMAGE_NFRAMES = 12


def damage_streams():
    """-> (frame lists, cfgs) of DAMAGE_CONFIGS: the oracle's frames of 12 frames of audio per stream"""
    cfgs = [dict(samplerate=fs, mode=mode, kbps=kbps, psy=psy, pad_len=0) for fs, mode, kbps, psy in DAMAGE_CONFIGS]
    assert {D.pick_table(c) for c in cfgs} == {0, 1, 2, 3, 4} and {D.dab_ext_of(c) for c in cfgs} == {2, 4}
    pcm = np.stack([signal_pcm(s, LOUD_SIGNALS[s % len(LOUD_SIGNALS)], DAMAGE_NFRAMES, 8800 + s) for s in range(len(cfgs))], axis=1)
    data, _ = oracle_sweep(cfgs, pcm)
    fl = [D.cut_frames(d, c) for d, c in zip(data, cfgs)]
    assert all(len(f) == DAMAGE_NFRAMES for f in fl)
    assert len({len(b) for b in fl[DAMAGE_PAD_STREAM]}) == 2      # it does have frames of both lengths
    return fl, cfgs
