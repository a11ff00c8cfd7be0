"""CPU checks of the one workspace description of the online decoders (csrc/online_api.cuh, OlWS / ol_carve): the byte totals of
every size query are pinned.  The four forms (folded, adaptive, multi-stream, adaptive multi-stream) take their blocks from one
carve, every block 256-aligned, so a total says which blocks a form has: one gained or lost by accident shows here before anything
runs on a GPU, and a caller that allocated by these numbers keeps working.  dtype order CP_F32, CP_BF16."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
PAIRS = [(1, 1), (3, 17), (7, 100), (256, 4096), (256, 65536)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def _dtypes():
    from contrastiveprosthetics_amd._lib import CP_BF16, CP_F32
    return CP_F32, CP_BF16


@pytest.mark.parametrize("entry,args,expected", [
    ("cp_online_workspace_bytes", [(m,) for m in (1, 16, 17, 256)],
     ([8055296, 8055296, 8137984, 9295616], [4041216, 4041216, 4082944, 4667136])),
    ("cp_online_adapt_workspace_bytes", [(m,) for m in (1, 16, 17, 256)],
     ([8359936, 8359936, 8639232, 12549376], [4272128, 4272128, 4436736, 6741248])),
    ("cp_online_multi_workspace_bytes", PAIRS,
     ([8055552, 8153600, 8597760, 31101184, 348623104], [4041472, 4098560, 4337920, 16642304, 176877824])),
    ("cp_online_multi_adapt_workspace_bytes", PAIRS,
     ([8360192, 8802304, 10524416, 100345344, 1172841984], [4272384, 4599808, 5748480, 67012096, 699106816])),
    ("cp_online_adapt_calibrate_scratch_bytes", [(n,) for n in (1, 2, 257, 5000)],
     ([3261440, 3266560, 4572160, 28856320], [2079232, 2081792, 2734592, 14876672])),
    ("cp_online_enroll_scratch_bytes", [(n,) for n in (1, 17, 256, 5000)],
     ([278528, 557056, 4456448, 4456448], [163840, 327680, 2621440, 2621440])),
])
def test_size_queries_return_the_bytes_they_always_returned(lib, entry, args, expected):
    for dt, want in zip(_dtypes(), expected):
        got = [getattr(lib, entry)(*a, dt) for a in args]
        assert got == want, (entry, dt, got, want)


def test_state_and_gate_sizes(lib):
    assert lib.cp_online_frontend_state_bytes() == 3328
    assert lib.cp_online_gate_workspace_bytes(1) == 2816
    assert lib.cp_online_gate_workspace_bytes(256) == 663552


def test_the_forms_nest_as_the_shared_entries_need(lib):
    """cp_online_set_classes / cp_online_reset take an adaptive workspace, cp_online_multi_set_classes / cp_online_multi_reset a
    multi-adaptive one: each checks the size of the folded form, so the adaptive form of the same shape is never the smaller"""
    for dt in _dtypes():
        for m in (1, 16, 17, 256):
            assert lib.cp_online_adapt_workspace_bytes(m, dt) >= lib.cp_online_workspace_bytes(m, dt)
        for s, r in PAIRS:
            assert lib.cp_online_multi_adapt_workspace_bytes(s, r, dt) >= lib.cp_online_multi_workspace_bytes(s, r, dt)
