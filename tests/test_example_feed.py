"""The examples with a Layer II feed (test 6 of the feed tests): `editick --feed FILE.mp2 --feed-bitrate K` ships the same AF packets as
`editick` on the decoded PCM of the same file, and `mp2enc --from-mp2` writes the same frames as `mp2enc` on that PCM.  The decoded PCM is
the existing Batch.decode's.  Every run of an example is under a time limit of its own."""
import subprocess

import numpy as np
import pytest

import declib as D
import feedlib as F
from pcmgen import gen_pcm
from test_example_mp2enc import build

pytestmark = pytest.mark.gpu
NFRAMES = 6
CASES = [(48000, 2, "s", 192, "j", 128), (24000, 1, "m", 64, "m", 64), (44100, 2, "j", 128, "s", 192)]      # rate, channels, the source's mode and kbps, the encoder's


def run(args):
    r = subprocess.run(["timeout", "-k", "10", "60"] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stderr


def make_source(tmp_path, fs, channels, mode, kbps):
    """-> (the .mp2 file, the raw interleaved PCM file the existing decoder makes of it)"""
    import odr_audioenc_amd as M
    b = M.Batch([M.StreamConfig(samplerate=fs, mode=mode, bitrate=kbps, psy_model=1)])
    data, _ = b.encode(gen_pcm(55, 0, 0, NFRAMES)[:, None])
    data = data[0] + b.flush()[0]
    frames = D.cut_frames(data, dict(samplerate=fs, kbps=kbps))
    assert len(frames) == NFRAMES
    fr, ln = D.batch_arrays([frames], b.out_stride)
    rep, _, planar = b.decode(fr, ln, False, True)
    b.close()
    assert not (rep["status"] & D.BAD_MASK).any() and np.abs(planar.astype(int)).max() > 1000
    (tmp_path / "src.mp2").write_bytes(data)
    (tmp_path / "dec.pcm").write_bytes(F.interleave(planar[:, 0], channels)[:, :1152 * channels].astype("<i2").tobytes())
    return tmp_path / "src.mp2", tmp_path / "dec.pcm"


@pytest.mark.parametrize("fs,channels,smode,skbps,mode,kbps", CASES[:2])
def test_editick_feed_ships_what_editick_ships_on_the_decoded_pcm(tmp_path, fs, channels, smode, skbps, mode, kbps):
    exe = build(tmp_path, "editick")
    mp2, pcm = make_source(tmp_path, fs, channels, smode, skbps)
    common = ["-r", fs, "-c", channels, "-b", kbps, "-m", mode, "-n", 3, "-t", 1712345678]
    err = run([exe, "-", tmp_path / "fed.af"] + common + ["--feed", mp2, "--feed-bitrate", skbps])
    assert f"{NFRAMES} frames of {skbps} kbps in the file, 0 feed frames did not pass" in err
    run([exe, pcm, tmp_path / "pcm.af"] + common)
    got = (tmp_path / "fed.af").read_bytes()
    assert got == (tmp_path / "pcm.af").read_bytes() and got.count(b"AF") >= NFRAMES


@pytest.mark.parametrize("fs,channels,smode,skbps,mode,kbps", CASES)
def test_mp2enc_from_mp2_equals_mp2enc_on_the_decoded_pcm(tmp_path, fs, channels, smode, skbps, mode, kbps):
    exe = build(tmp_path)
    mp2, pcm = make_source(tmp_path, fs, channels, smode, skbps)
    err = run([exe, mp2, tmp_path / "a.mp2", "--from-mp2", "-b", kbps, "-m", mode, "-n", 2])
    assert f"transcoded from {fs} Hz, {skbps} kbps, {channels} channel(s): {NFRAMES} frames, 0 did not pass" in err
    run([exe, pcm, tmp_path / "b.mp2", "-r", fs, "-c", channels, "-b", kbps, "-m", mode, "-n", 2])
    got = (tmp_path / "a.mp2").read_bytes()
    assert got == (tmp_path / "b.mp2").read_bytes() and len(D.cut_frames(got, dict(samplerate=fs, kbps=kbps))) == NFRAMES


def test_nodetick_feed_ships_what_a_tick_object_ships(tmp_path):
    """`nodetick --feed` over two shards on one GPU: the AF packets of the LAST service equal a single Tick object's fed the same frames,
    and a run with one shard ships the same bytes"""
    import json
    import struct
    import odr_audioenc_amd as M
    exe = build(tmp_path, "nodetick")
    mp2, _ = make_source(tmp_path, 48000, 2, "s", 192)
    frames = D.cut_frames(mp2.read_bytes(), dict(samplerate=48000, kbps=192))
    ns, ticks = 9, 8
    outs = {}
    for d in ("0,0", "0"):
        r = subprocess.run(["timeout", "-k", "10", "60", str(exe), "-", "-n", str(ns), "-d", d, "-k", str(ticks), "-o", str(tmp_path / f"out_{len(d)}.af"),
                            "--feed", str(mp2), "--feed-bitrate", "192"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs[d] = json.loads(r.stdout.strip().splitlines()[-1])
    assert outs["0,0"]["shards"] == 2 and outs["0,0"]["packets"] == outs["0"]["packets"] == ns * ticks and outs["0,0"]["bytes"] == outs["0"]["bytes"]
    blob, got, o = (tmp_path / "out_3.af").read_bytes(), [], 0
    assert (tmp_path / "out_1.af").read_bytes() == blob
    while o < len(blob):
        k = struct.unpack_from("<I", blob, o)[0]
        got.append(blob[o + 4:o + 4 + k])
        o += 4 + k
    t = M.Tick([M.StreamConfig(mode="j", bitrate=128, psy_model=1)], egress="af", version=b"nodetick example", now_s=1712345678, delay_ms=0, tist=True, tai_utc_offset=37)
    t.set_feed(0, M.FeedConfig(48000, 192, 2))
    want = []
    for f in range(ticks):
        b = frames[(ns - 1 + f) % len(frames)]
        t.feed[0, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        t.feed_len[0] = len(b)
        t.run()
        want += t.packets(0)
    t.finish()
    want += t.packets(0)
    t.close()
    assert got == want and len(got) == ticks
