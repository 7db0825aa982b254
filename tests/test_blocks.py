"""The cut of N streams into G blocks and the routing of a stream id to its block (csrc/tlb_blocks.h), CPU only: the header the node's shards
and a tick object's stream groups both come from, walked over every small (N, G) under AddressSanitizer and UBSan (tests/emu/blocks_main.cpp).
The program is linked with the sanitizers; nothing is preloaded.  tests/test_node_plan.py pins the same cut through the library's
tlb_node_partition()."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_cut_owner_and_visits_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "blocks_main"
    src = ROOT / "tests" / "emu" / "blocks_main.cpp"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "blocks ok: 326 cases" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])

