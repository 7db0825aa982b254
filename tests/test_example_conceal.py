"""The examples with feed concealment: `editick --feed ... --feed-drop-every 5 --feed-drop-run 2 --conceal` prints the record the drop
pattern implies and ships what a tick object with concealment ships; without --conceal the same run ships what a tick object WITHOUT
concealment ships for the same empty slots (the behaviour before concealment existed: silence); `nodetick` and `mp2enc --from-mp2` take
the option too.  Every run of an example is under a time limit of its own."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import conceallib as K
import declib as D
from pcmgen import gen_pcm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NFRAMES, NS, EVERY, RUN = 12, 3, 5, 2
DROPPED = [f % EVERY >= EVERY - RUN for f in range(NFRAMES)]     # ticks 3, 4, 8, 9


def build(tmp_path, name):
    """the example against the library as it stands (built when there is none)"""
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "examples" / (name + ".cpp")), "-I" + str(ROOT / "include"),
                    "-L" + str(ROOT / "odr-audioenc_amd"), "-ltoolame_dab_hip", "-Wl,-rpath," + str(ROOT / "odr-audioenc_amd"), "-pthread", "-o", str(exe)], check=True)
    return exe


def run(args):
    r = subprocess.run(["timeout", "-k", "10", "60"] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    """twelve frames, 48 kHz stereo 192 kbps -> (the .mp2 file, its frames)"""
    import odr_audioenc_amd as M
    b = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=192, psy_model=1)])
    data, _ = b.encode(gen_pcm(56, 0, 0, NFRAMES)[:, None])
    data = data[0] + b.flush()[0]
    b.close()
    frames = D.cut_frames(data, dict(samplerate=48000, kbps=192))
    assert len(frames) == NFRAMES
    path = tmp_path_factory.mktemp("concealsrc") / "src.mp2"
    path.write_bytes(data)
    return path, frames


def af_packets(path):
    blob, out, o = Path(path).read_bytes(), [], 0
    while o < len(blob):
        k = struct.unpack_from("<I", blob, o)[0]
        out.append(blob[o + 4:o + 4 + k])
        o += 4 + k
    return out


def tick_packets(frames, conceal, stream, version):
    """what one tick object ships for service `stream` of the examples: frame (tick + stream) of the file, the dropped ticks' slots empty"""
    import odr_audioenc_amd as M
    t = M.Tick([M.StreamConfig(mode="j", bitrate=128, psy_model=1)], egress="af", version=version, now_s=1712345678, delay_ms=0, tist=True, tai_utc_offset=37)
    t.set_feed(0, M.FeedConfig(48000, 192, 2))
    if conceal:
        t.enable_conceal(4, 3)
    out = []
    for f in range(NFRAMES):
        if not DROPPED[f]:
            b = frames[(f + stream) % len(frames)]
            t.feed[0, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            t.feed_len[0] = len(b)
        t.run()
        out += t.packets(0)
    t.finish()
    out += t.packets(0)
    t.close()
    return out


def want_line(ns):
    rec = K.oracle_record(DROPPED, 4, 3)
    assert [int(rec[n]) for n in ("frames", "passed", "concealed", "muted", "runs", "longest")] == [12, 8, 4, 0, 2, 2]
    return "conceal: %d slots, %d passed, %d concealed, %d muted, %d runs, longest %d" % (ns * 12, ns * 8, ns * 4, 0, ns * 2, 2)


def test_editick_conceals_what_the_drop_pattern_loses(tmp_path, source):
    mp2, frames = source
    exe = build(tmp_path, "editick")
    common = ["-n", NS, "-t", 1712345678, "--feed", mp2, "--feed-bitrate", 192, "--feed-drop-every", EVERY, "--feed-drop-run", RUN]
    r = run([exe, "-", tmp_path / "on.af"] + common + ["--conceal"])
    assert "editick: " + want_line(NS) in r.stderr, r.stderr
    assert f"{NFRAMES} ticks of {NS} stream(s)" in r.stderr
    r = run([exe, "-", tmp_path / "off.af"] + common)
    assert "conceal:" not in r.stderr
    on, off = af_packets(tmp_path / "on.af"), af_packets(tmp_path / "off.af")
    assert off == tick_packets(frames, False, 0, b"editick example") and len(off) == NFRAMES      # without --conceal: what it shipped before
    assert on == tick_packets(frames, True, 0, b"editick example") and on != off
    r = run([exe, "-", tmp_path / "h2.af"] + common + ["--conceal", 1, "--conceal-step", 21])     # hold 1: the second lost frame of each run rings out
    assert "editick: " + want_line(NS) in r.stderr and af_packets(tmp_path / "h2.af") != on
    bad = subprocess.run(["timeout", "-k", "10", "60", str(exe), str(mp2), str(tmp_path / "x.af"), "--conceal"], capture_output=True, text=True)
    assert bad.returncode == 1 and "strict --feed" in bad.stderr  # no feed: refused before anything runs


def test_nodetick_and_mp2enc_take_the_option(tmp_path, source):
    mp2, frames = source
    exe = build(tmp_path, "nodetick")
    r = run([exe, "-", "-n", NS, "-d", "0", "-k", NFRAMES, "-o", tmp_path / "node.af", "--feed", mp2, "--feed-bitrate", 192,
             "--feed-drop-every", EVERY, "--feed-drop-run", RUN, "--conceal"])
    assert "nodetick: " + want_line(NS) in r.stderr, r.stderr
    assert af_packets(tmp_path / "node.af") == tick_packets(frames, True, NS - 1, b"nodetick example")       # -o: the LAST service's packets
    # mp2enc --from-mp2 --conceal on a file whose frames 3 and 4 have a damaged CRC-16
    hurt = [bytes(bytearray(b[:5]) + bytes([b[5] ^ 1]) + b[6:]) if f in (3, 4) else b for f, b in enumerate(frames)]
    (tmp_path / "hurt.mp2").write_bytes(b"".join(hurt))
    exe = build(tmp_path, "mp2enc")
    r = run([exe, tmp_path / "hurt.mp2", tmp_path / "a.mp2", "--from-mp2", "-b", 128, "--conceal"])
    assert "12 frames, 2 did not pass" in r.stderr and "mp2enc: conceal: 12 slots, 10 passed, 2 concealed, 0 muted, 1 runs, longest 2" in r.stderr, r.stderr
    run([exe, tmp_path / "hurt.mp2", tmp_path / "b.mp2", "--from-mp2", "-b", 128])
    a, b = (tmp_path / "a.mp2").read_bytes(), (tmp_path / "b.mp2").read_bytes()
    assert len(a) == len(b) and a != b and len(D.cut_frames(a, dict(samplerate=48000, kbps=128))) == NFRAMES
