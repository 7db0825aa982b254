"""ThreadSanitizer on the timed join of the node's threading primitive (csrc/tlb_mailbox.h: join_job_until, poll, busy), CPU only: fake
jobs in the node's patterns under a tick deadline (tests/emu/mailbox_deadline_tsan.cpp) -- jobs inside the deadline, jobs held past it
(the poster must see `false` while the job provably runs, then poll() its code later), late jobs that return an error, jobs that own
what they use because the frame that posted them has returned, and counter reads by the poster while a late job runs.  Sanitizers
belong on the CPU build."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_mailbox_deadline_is_clean_under_threadsanitizer(tmp_path):
    exe = tmp_path / "mailbox_deadline_tsan"
    src = ROOT / "tests" / "emu" / "mailbox_deadline_tsan.cpp"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=300, env={"TSAN_OPTIONS": "halt_on_error=1 exitcode=66"})
    print(r.stdout)
    assert r.returncode == 0 and "mailbox deadline ok" in r.stdout and "ThreadSanitizer" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
