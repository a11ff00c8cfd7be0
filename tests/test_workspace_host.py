"""CPU checks of the training encoder's workspace description (csrc/encoder_api.cuh, WS / carve) and the glove-angle class encoder's
(csrc/api.hip, GWS / carve_glove): the byte totals of both size queries are pinned.  Every block is 256-aligned and taken from one
carve, so a total says which blocks a configuration has -- one gained or lost by accident shows here before anything runs on a GPU,
and a caller that allocated by these numbers keeps working.  The values were recorded from the library before the encoder's host layer
moved out of api.hip.  N: one group, the last small-batch size, the first large-batch size, the benchmark's batch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
WINDOWS = (41, 2624, 2665, 167936)

# dtype -> (cp_workspace_bytes at dp 0, at dp 0.0635, cp_glove_workspace_bytes), one value per entry of WINDOWS
TABLE = {
    "CP_F32": ([105938688, 167558656, 168536832, 4111241728], [173639424, 272289280, 273855232, 6585885184],
               [21593600, 30851072, 30998016, 623329280]),
    "CP_BF16": ([97438976, 128310784, 128801024, 2104119808], [164845824, 214232576, 215016704, 3374998016],
                [21438464, 26066944, 26140672, 322306048]),
    "CP_FP8": ([101601536, 146359552, 147070208, 3010885888], [169008384, 232281344, 233285888, 4281764096],
               [21438464, 26066944, 26140672, 322306048]),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("dtype", sorted(TABLE))
def test_size_queries_return_the_bytes_they_always_returned(lib, dtype):
    from contrastiveprosthetics_amd import _lib
    dt = getattr(_lib, dtype)
    plain, dropout, glove = TABLE[dtype]
    assert [lib.cp_workspace_bytes(n, dt, 0.0) for n in WINDOWS] == plain
    assert [lib.cp_workspace_bytes(n, dt, 0.0635) for n in WINDOWS] == dropout
    assert [lib.cp_glove_workspace_bytes(n, dt) for n in WINDOWS] == glove


def test_no_rows_no_bytes(lib):
    from contrastiveprosthetics_amd import _lib
    assert lib.cp_workspace_bytes(0, _lib.CP_BF16, 0.0) == 0 and lib.cp_workspace_bytes(-41, _lib.CP_BF16, 0.0) == 0
    assert lib.cp_glove_workspace_bytes(0, _lib.CP_BF16) == 0 and lib.cp_glove_workspace_bytes(41, 7) == 0
