"""The resampler's C-ABI without a GPU: the names are declared and exported, tlb_resample_need_at's arithmetic, NULL handles."""
import ctypes as C
import re
from pathlib import Path

import pytest

import resamplelib as R

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["tlb_resample_set_source", "tlb_resample_source", "tlb_resample_need", "tlb_resample_need_at", "tlb_resample_taps", "tlb_resample_device",
         "tlb_resample_host", "tlb_tick_set_source", "tlb_tick_need", "tlb_node_set_source", "tlb_node_need"]
ERR_SAMPLERATE, ERR_ARG = 1, 18


def lib():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M.load_library()


def test_names_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "toolame_batch.h").read_text(), flags=re.S)
    L = lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n), n


@pytest.mark.parametrize("pair", [(44100, 48000), (22050, 24000)])
def test_need_cycle_of_five(pair):
    import odr_audioenc_amd as M
    got = [M.resample_need_at(pair[0], pair[1], f) for f in range(40)]
    assert set(got) == {1058, 1059}
    for f in range(35):
        assert sum(got[f:f + 5]) == 5292
    assert got == [R.need(pair[0], pair[1], f) for f in range(40)]      # the header's formula in Python ints
    assert got[:5] == got[5:10]
    assert M.resample_need_at(pair[0], pair[1], 10 ** 9 + 3) == got[3]


@pytest.mark.parametrize("pair", [(32000, 48000), (16000, 24000)])
def test_need_is_768_for_three_halves(pair):
    import odr_audioenc_amd as M
    assert [M.resample_need_at(pair[0], pair[1], f) for f in range(12)] == [768] * 12


def test_unsupported_pairs():
    L = lib()
    for pair in ((48000, 24000), (48000, 44100), (44100, 24000)):
        assert L.tlb_resample_need_at(pair[0], pair[1], 0) == -ERR_SAMPLERATE
    assert L.tlb_resample_need_at(44100, 48000, -1) == -ERR_ARG


def test_null_handles():
    L = lib()
    assert L.tlb_resample_set_source(None, 0, 44100) == ERR_ARG
    assert L.tlb_resample_source(None, 0) == 0
    assert L.tlb_resample_need(None, 0, 0) == -ERR_ARG
    assert L.tlb_resample_device(None, None, 1, None, None) == ERR_ARG
    assert L.tlb_resample_host(None, None, 1, None) == ERR_ARG
    assert L.tlb_tick_set_source(None, 0, 44100) == ERR_ARG
    assert L.tlb_tick_need(None, 0) == -ERR_ARG
    assert L.tlb_node_set_source(None, 0, 44100) == ERR_ARG
    assert L.tlb_node_need(None, 0) == -ERR_ARG
    assert L.tlb_resample_taps(44100, 48000, None, None, None)
    assert not L.tlb_resample_taps(48000, 44100, None, None, None)
