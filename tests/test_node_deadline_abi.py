"""The tick deadline's names in the libraries' export tables (CPU only, no GPU): the product library exports the new public entry points
include/toolame_batch.h declares and no stall hook; the fault-injection TEST build has the hook (csrc/tlb_debug.h)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW_PUBLIC = ("tlb_node_set_deadline_ms", "tlb_node_shard_deadline_status")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def _built():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists() or not M.FAULT_LIB_PATH.exists():
        M.build()
    return M


def test_product_exports_the_deadline_api_and_no_stall_hook():
    M = _built()
    names = _exports(M.LIB_PATH)
    for n in NEW_PUBLIC:
        assert n in names, n
    assert "tlb_debug_node_stall_next" not in names
    assert not any(n.startswith("tlb_debug_") for n in names)


def test_header_declares_the_deadline_api():
    text = (ROOT / "include" / "toolame_batch.h").read_text()
    for n in NEW_PUBLIC + ("tlb_node_shard_deadline", "TLB_ERR_LATE = 19", "TLB_SHARD_LATE 2"):
        assert n in text, n


def test_fault_build_has_the_stall_hook():
    M = _built()
    names = _exports(M.FAULT_LIB_PATH)
    assert "tlb_debug_node_stall_next" in names
    for n in NEW_PUBLIC:
        assert n in names, n
