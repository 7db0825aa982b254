"""The examples with a DOWN FEED: `mp2enc --from-mp2 -r 24000` on a 48 kHz file writes the frames `mp2enc` writes on the oracle's PCM (the
existing decoder's samples and the decimator's formula in numpy), `editick -r 24000 --feed .. --feed-rate 48000` ships what `editick -r
24000 --source-rate 48000` ships on the decoded PCM, and `nodetick` ships over two shards what it ships over one.  Every run of an example
is under a time limit of its own."""
import numpy as np
import pytest

import declib as D
import feeddownlib as A
import feedlib as F
from pcmgen import gen_pcm
from test_example_feed import run
from test_example_mp2enc import build

pytestmark = pytest.mark.gpu
NFRAMES = 12                                                         # six ticks at 24 kHz: two feed frames each
FS, KBPS = 48000, 192


def make_source(tmp_path):
    """-> (the 48 kHz stereo .mp2 file, its decoded source frames int16 [NFRAMES * 1152][2] as the existing decoder makes them)"""
    import odr_audioenc_amd as M
    b = M.Batch([M.StreamConfig(samplerate=FS, mode="s", bitrate=KBPS, psy_model=1)])
    data, _ = b.encode(gen_pcm(57, 0, 0, NFRAMES)[:, None])
    data = data[0] + b.flush()[0]
    frames = D.cut_frames(data, dict(samplerate=FS, kbps=KBPS))
    assert len(frames) == NFRAMES
    fr, ln = D.batch_arrays([frames], b.out_stride)
    rep, _, planar = b.decode(fr, ln, False, True)
    b.close()
    assert not (rep["status"] & D.BAD_MASK).any() and np.abs(planar.astype(int)).max() > 1000
    (tmp_path / "src.mp2").write_bytes(data)
    return tmp_path / "src.mp2", F.interleave(planar[:, 0], 2).reshape(-1, 2)


def test_mp2enc_from_mp2_above_the_encoders_rate(tmp_path):
    exe = build(tmp_path)
    mp2, x = make_source(tmp_path)
    nticks = NFRAMES // 2
    want = A.oracle_ticks(x, FS, 2, 2, nticks)
    (tmp_path / "oracle.pcm").write_bytes(want.astype("<i2").tobytes())
    err = run([exe, mp2, tmp_path / "a.mp2", "--from-mp2", "-r", 24000, "-b", 64, "-m", "s", "-n", 2])
    assert f"transcoded from {FS} Hz, {KBPS} kbps, 2 channel(s): {NFRAMES} frames, 0 did not pass" in err
    run([exe, tmp_path / "oracle.pcm", tmp_path / "b.mp2", "-r", 24000, "-b", 64, "-m", "s", "-n", 2])
    got = (tmp_path / "a.mp2").read_bytes()
    assert got == (tmp_path / "b.mp2").read_bytes() and len(D.cut_frames(got, dict(samplerate=24000, kbps=64))) == nticks


def test_editick_down_feed_ships_what_editick_ships_with_a_down_source(tmp_path):
    exe = build(tmp_path, "editick")
    mp2, x = make_source(tmp_path)
    (tmp_path / "dec.pcm").write_bytes(x.astype("<i2").tobytes())
    common = ["-r", 24000, "-c", 2, "-b", 64, "-m", "s", "-n", 2, "-t", 1712345678]
    err = run([exe, "-", tmp_path / "fed.af"] + common + ["--feed", mp2, "--feed-bitrate", KBPS, "--feed-rate", FS])
    assert f"{NFRAMES} frames of {KBPS} kbps in the file, 0 feed frames did not pass" in err and f"{NFRAMES // 2} ticks of 2 stream(s)" in err
    err = run([exe, tmp_path / "dec.pcm", tmp_path / "pcm.af"] + common + ["--source-rate", FS])
    assert f"{NFRAMES // 2} ticks of 2 stream(s)" in err
    got = (tmp_path / "fed.af").read_bytes()
    assert got == (tmp_path / "pcm.af").read_bytes() and got.count(b"AF") >= NFRAMES // 2


def test_nodetick_down_feed_over_two_shards_ships_what_one_shard_ships(tmp_path):
    """`nodetick -r 24000 --feed .. --feed-rate 48000` over two shards on one GPU ships the bytes a run with one shard ships (the schedule is
    per stream, wherever the stream lives)"""
    import json
    import subprocess
    exe = build(tmp_path, "nodetick")
    mp2, _ = make_source(tmp_path)
    ns, ticks = 5, 7
    outs = {}
    for d in ("0,0", "0"):
        r = subprocess.run(["timeout", "-k", "10", "60", str(exe), "-", "-n", str(ns), "-d", d, "-k", str(ticks), "-r", "24000", "-b", "64", "-o", str(tmp_path / f"out_{len(d)}.af"),
                            "--feed", str(mp2), "--feed-bitrate", str(KBPS), "--feed-rate", str(FS)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs[d] = json.loads(r.stdout.strip().splitlines()[-1])
    assert outs["0,0"]["shards"] == 2 and outs["0,0"]["packets"] == outs["0"]["packets"] > 0 and outs["0,0"]["bytes"] == outs["0"]["bytes"]
    assert (tmp_path / "out_3.af").read_bytes() == (tmp_path / "out_1.af").read_bytes()
