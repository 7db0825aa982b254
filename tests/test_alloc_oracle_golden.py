"""The oracle of the allocation probe (tests/probelib.py alloc_greedy: a_bit_allocation_new with maxmnr_new restated event by event) against
the REFERENCE's own bit_alloc taps: on every golden that carries smr, scfsi, bit_alloc, mode and mode_ext and has no X-PAD, the oracle fed
the file's SMRs and scfsi gives the file's bit_alloc for every frame.  jsbound comes from the frame's mode / mode_ext taps (what the
joint-stereo trial loop chose), the bit budget from the configuration: 8 * frame bytes less the ScF-CRC bytes and the two F-PAD bytes
(toolame.c:292-301).  At 44.1 and 22.05 kHz a frame is one slot longer when its header's padding bit is set; the bit is read from the
reference's own byte stream (tests/declib.py cut_frames: frame i of the stream is frame i of the taps, which tests/test_decode_emu.py
shows field by field), so the padded rates are covered without a guess.

No GPU, and nothing of csrc/ but the Layer II tables: this is what lets tests/test_probe_emu.py and tests/test_probe_gpu.py call the oracle
the reference."""
import numpy as np

import declib as D
import probelib as P

TAPS = ("smr", "scfsi", "bit_alloc", "mode", "mode_ext")


def test_oracle_gives_the_references_bit_alloc_on_every_golden_frame():
    T = P._alloc_tables()
    tab, nch, jsb, adb, smr, sel, want, where = [], [], [], [], [], [], [], []
    for name in D.golden_names():
        g = np.load(D.GOLDEN / (name + ".npz"))
        cfg = D.golden_cfg(g)
        if cfg["pad_len"] or not all(k in g.files for k in TAPS):
            continue
        t, n = D.pick_table(cfg), 1 if cfg["mode"] == "m" else 2
        frames = D.cut_frames(g["data"], cfg)
        nf = g["bit_alloc"].shape[0]
        assert len(frames) >= nf
        for f in range(nf):
            mode, ext = int(g["mode"][f]), int(g["mode_ext"][f])
            assert (frames[f][3] >> 6) == mode and ((frames[f][3] >> 4) & 3) == ext, "%s: frame %d of the stream is not frame %d of the taps" % (name, f, f)
            tab.append(t); nch.append(n)
            jsb.append(4 * (ext + 1) if mode == 1 else int(T["sblimit"][t]))
            adb.append(8 * len(frames[f]) - 8 * (D.dab_ext_of(cfg) + 2))
            smr.append(g["smr"][f]); sel.append(g["scfsi"][f]); want.append(g["bit_alloc"][f]); where.append((name, f))
    R = P.alloc_greedy(np.array(tab), np.array(nch), np.array(jsb), np.array(adb), np.array(smr), np.array(sel))
    want = np.array(want).astype(np.int64)
    bad = np.argwhere(R["ba"] != want)
    assert not bad.size, "%s frame %d: channel %d subband %d: oracle %d, reference %d (%d cells of %d frames differ)" % (
        where[bad[0][0]] + (bad[0][1], bad[0][2], R["ba"][tuple(bad[0])], want[tuple(bad[0])], bad.shape[0], np.unique(bad[:, 0]).size))
    rates = {D.golden_cfg(np.load(D.GOLDEN / (nm + ".npz")))["samplerate"] for nm, _ in where}
    assert len(where) >= 1700 and rates == {48000, 44100, 32000, 24000, 22050, 16000}, (len(where), rates)      # no silent skip hollows it out
    assert (np.array(jsb) < T["sblimit"][np.array(tab)]).sum() > 50                                                # joint frames among them
