"""CPU checks of the electrode map (contrastiveprosthetics_amd/online.py set_channel_map, rotations, leave_one_out,
score_channel_maps, pick_channel_map; csrc/online_maps.cuh): the candidate maps, what the Python side refuses, the C entries'
declarations, sizes and refusals before any device call, and the tie order of the pick."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG = 10001
MAPPED = ["cp_online_push_mapped", "cp_online_adapt_push_mapped", "cp_online_multi_push_mapped", "cp_online_multi_adapt_push_mapped",
          "cp_online_windows_mapped"]
SWEEP = ["cp_online_map_sweep_scratch_bytes", "cp_online_map_sweep", "cp_online_adapt_map_sweep", "cp_online_multi_map_sweep",
         "cp_online_multi_adapt_map_sweep"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------
# candidate maps
# ---------------------------------------------------------------------------------------------------------------------------
def test_rotations_are_the_cyclic_shifts_of_the_ring():
    from contrastiveprosthetics_amd.online import rotations
    r = rotations()
    assert r.shape == (8, 12) and r.dtype == np.int32
    assert r[0].tolist() == list(range(12))                              # shift 0 is the identity
    assert len({tuple(m) for m in r}) == 8
    for s in range(8):
        assert r[s, 8:].tolist() == [8, 9, 10, 11]                       # the channels off the ring stay
        assert r[s, :8].tolist() == [(i + s) % 8 for i in range(8)]
        assert sorted(r[s].tolist()) == list(range(12))                  # a permutation
    # a rotation and the opposite one undo each other: raw[:, r[3]][:, r[5]] == raw
    assert r[3][r[5]].tolist() == list(range(12))


def test_reflected_rotations_and_another_ring():
    from contrastiveprosthetics_amd.online import rotations
    r = rotations(reflect=True)
    assert r.shape == (16, 12) and len({tuple(m) for m in r}) == 16
    assert (r[:8] == rotations()).all()
    for s in range(8):
        assert r[8 + s, 8:].tolist() == [8, 9, 10, 11]
        assert r[8 + s, :8].tolist() == [(s - i) % 8 for i in range(8)]
    ring = (2, 5, 11, 7)                                                 # a sleeve with four electrodes around the arm
    q = rotations(ring)
    assert q.shape == (4, 12) and q[0].tolist() == list(range(12))
    assert [int(q[1, c]) for c in ring] == [5, 11, 7, 2]
    off = [c for c in range(12) if c not in ring]
    assert (q[:, off] == np.array(off)).all()
    for bad in ((0,), (0, 0, 1), (0, 12), (-1, 2)):
        with pytest.raises(ValueError, match="ring"):
            rotations(bad)


def test_leave_one_out_masks_one_channel_each():
    from contrastiveprosthetics_amd.online import leave_one_out
    m = leave_one_out()
    assert m.shape == (12, 12) and m.dtype == np.int32
    for d in range(12):
        want = list(range(12))
        want[d] = -1
        assert m[d].tolist() == want


# ---------------------------------------------------------------------------------------------------------------------------
# what the Python side refuses
# ---------------------------------------------------------------------------------------------------------------------------
def test_check_map_refuses_bad_maps():
    from contrastiveprosthetics_amd.online import _check_map
    assert _check_map(None) is None
    src, fill = _check_map(list(range(12)))
    assert src.dtype == np.int32 and src.tolist() == list(range(12)) and fill.dtype == np.float32 and fill.tolist() == [0.0] * 12
    src, fill = _check_map([4] * 11 + [-1], 0.25)                        # no permutation, one fill for all
    assert src.tolist() == [4] * 11 + [-1] and fill.tolist() == [0.25] * 12
    with pytest.raises(ValueError, match="12 entries"):
        _check_map(list(range(11)))
    with pytest.raises(ValueError, match="12 entries"):
        _check_map(list(range(13)))
    with pytest.raises(ValueError, match="12 entries"):
        _check_map(np.zeros((12, 1), dtype=int))
    with pytest.raises(ValueError, match="-1..11"):
        _check_map([0] * 11 + [12])
    with pytest.raises(ValueError, match="-1..11"):
        _check_map([-2] + [0] * 11)
    with pytest.raises(ValueError, match="integers"):
        _check_map([0.5] * 12)
    with pytest.raises(ValueError, match="finite"):
        _check_map(list(range(12)), [0.0] * 11 + [float("nan")])
    with pytest.raises(ValueError, match="finite"):
        _check_map(list(range(12)), float("inf"))
    with pytest.raises(ValueError, match="fill"):
        _check_map(list(range(12)), [0.0] * 5)
    with pytest.raises(ValueError, match="fill"):
        _check_map(None, 0.5)


def test_map_windows_overwrites_the_masked_columns_only():
    import torch
    from contrastiveprosthetics_amd.online import _check_map, _map_windows
    w = torch.arange(36, dtype=torch.float32).reshape(3, 12)
    src = list(range(12))
    src[2] = src[9] = -1
    fill = [0.0] * 12
    fill[9] = 0.25
    fill[4] = 7.0                                                        # not masked: never read
    out = _map_windows(w.clone(), _check_map(src, fill))
    assert out[:, 2].tolist() == [0.0] * 3 and out[:, 9].tolist() == [0.25] * 3
    keep = [c for c in range(12) if c not in (2, 9)]
    assert torch.equal(out[:, keep], w[:, keep])


# ---------------------------------------------------------------------------------------------------------------------------
# the pick
# ---------------------------------------------------------------------------------------------------------------------------
def test_pick_channel_map_orders_by_voted_raw_index():
    from contrastiveprosthetics_amd.online import pick_channel_map

    def s(v, r):
        return dict(rows=100, raw_hits=r, voted_hits=v)

    assert pick_channel_map([s(5, 9), s(7, 1), s(6, 9)]) == 1            # the most voted hits
    assert pick_channel_map([s(7, 1), s(7, 3), s(7, 2)]) == 1            # then the most raw hits
    assert pick_channel_map([s(7, 3), s(7, 3), s(2, 9)]) == 0            # then the lowest index
    assert pick_channel_map([s(0, 0)]) == 0
    with pytest.raises(ValueError):
        pick_channel_map([])


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
def test_map_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import MAP_SCORE_KEYS
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in MAPPED + SWEEP:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    # a mapped entry takes its twin's arguments and the two map pointers
    for n in MAPPED:
        assert len(_lib.SYMBOLS[n][1]) == len(_lib.SYMBOLS[n.replace("_mapped", "")][1]) + 2, n
    assert int(re.search(r"#define\s+CP_ONLINE_MAP_SCORES\s+(\d+)", hdr).group(1)) == _lib.CP_ONLINE_MAP_SCORES == len(MAP_SCORE_KEYS) == 3
    assert int(re.search(r"#define\s+CP_ONLINE_MAP_SWEEP_MAX_MAPS\s+(\d+)", hdr).group(1)) == _lib.CP_ONLINE_MAP_SWEEP_MAX_MAPS == 65536
    assert lib.cp_version() == 112
    assert lib.cp_online_frontend_state_bytes() == 3328                  # the map lives outside the state


def test_sweep_scratch_is_monotone_in_rows_and_bounded_by_the_chunk(lib):
    f = lib.cp_online_map_sweep_scratch_bytes
    for dtype in (0, 1):
        for adaptive in (0, 1):
            last = 0
            for n in (1, 15, 16, 17, 300, 6321, 16384, 16385, 10 ** 6, 2 ** 31 - 1):
                b = f(n, 0, dtype, adaptive)
                assert b >= last and b % 256 == 0, (n, dtype, adaptive)
                last = b
            assert f(10 ** 6, 0, dtype, adaptive) == f(2 ** 31 - 1, 0, dtype, adaptive)     # one chunk, however many rows
            assert f(10 ** 6, 48, dtype, adaptive) < f(10 ** 6, 1000, dtype, adaptive) < f(10 ** 6, 0, dtype, adaptive)
            assert f(300, 1000, dtype, adaptive) == f(300, 0, dtype, adaptive)             # a chunk is never more than the rows
            assert f(0, 0, dtype, adaptive) == f(1, 0, dtype, adaptive)
        assert f(6321, 0, dtype, 1) > f(6321, 0, dtype, 0)                # conv2's operand and output of one piece
    es = 4
    rows = 6336                                                           # 6321 rounded up to whole tiles
    assert f(6321, 0, 0, 0) >= rows * (12 * 4 + 768 * es + 512 * es)


def _config(vote=25, dtype=0):
    from contrastiveprosthetics_amd.online import _config as make, _filter
    b, a = _filter(None, None)
    return make("f32" if dtype == 0 else "bf16", 256, vote, 0, b, a)


def test_sweep_refuses_bad_arguments_before_any_device_call(lib):
    """host memory in every pointer: each refusal returns before a launch, which on this machine would fail differently"""
    M, G, K = 10, 3, 8
    ws_bytes = lib.cp_online_workspace_bytes(256, 0)
    ws = 1 << 20                                                          # an aligned address nobody reads before the refusal
    rms = (ctypes.c_float * (M * 12))()
    ms = (ctypes.c_float * 24)()
    src = (ctypes.c_int32 * (G * 12))()
    fill = (ctypes.c_float * (G * 12))()
    exp = (ctypes.c_int32 * M)()
    pred = (ctypes.c_int32 * (G * M))()
    scores = (ctypes.c_int64 * (3 * G))()
    need = lib.cp_online_map_sweep_scratch_bytes(G * M, 0, 0, 0)
    scratch = 1 << 21
    good = dict(cfg=_config(), ws=ws, ws_bytes=ws_bytes, n_windows=M, n_maps=G, n_classes=K, chunk=0, scratch=scratch, need=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cp_online_map_sweep(ctypes.byref(a["cfg"]), a["ws"], a["ws_bytes"], rms, a["n_windows"], ms, src, fill, a["n_maps"],
                                       a["n_classes"], exp, a["chunk"], a["scratch"], a["need"], pred, None, scores, None, None)

    def refused(what, **kw):
        rc = call(**kw)
        assert rc == ERR_ARG, (kw, rc)
        msg = lib.cp_last_error()
        assert what.encode() in msg, (kw, msg)

    refused("workspace", ws=None)
    refused("n_maps", n_maps=0)
    refused("n_maps", n_maps=65537)
    refused("vote", cfg=_config(vote=0))
    refused("vote", cfg=_config(vote=257))
    refused("n_classes", n_classes=65)
    refused("n_classes", n_classes=0)
    refused("n_windows", n_windows=0)
    refused("2^31", n_windows=2 ** 31 // 3 + 1)
    refused("chunk_rows", chunk=-1)
    refused("not 256-byte aligned", ws=ws + 4)
    for name in ("cp_online_map_sweep", ):
        refused(name, n_maps=0)
    # the twins refuse in their own name
    rc = lib.cp_online_adapt_map_sweep(ctypes.byref(good["cfg"]), ws, ws_bytes, rms, M, ms, src, fill, 0, K, exp, 0, scratch, need, pred,
                                       None, scores, None, None)
    assert rc == ERR_ARG and b"cp_online_adapt_map_sweep" in lib.cp_last_error()
    for fn, who in ((lib.cp_online_multi_map_sweep, b"cp_online_multi_map_sweep"),
                    (lib.cp_online_multi_adapt_map_sweep, b"cp_online_multi_adapt_map_sweep")):
        rc = fn(ctypes.byref(good["cfg"]), 3, 256, ws, 1 << 40, 1, rms, M, ms, src, fill, G, 65, exp, 0, scratch, need, pred, None, scores,
                None, None)
        assert rc == ERR_ARG and who in lib.cp_last_error() and b"n_classes" in lib.cp_last_error()
        rc = fn(ctypes.byref(good["cfg"]), 3, 256, ws, 1 << 40, 3, rms, M, ms, src, fill, G, K, exp, 0, scratch, need, pred, None, scores,
                None, None)
        assert rc == ERR_ARG and b"stream index" in lib.cp_last_error()


def test_mapped_entries_refuse_half_a_map_before_any_device_call(lib):
    """both map pointers or neither; the refusal names the mapped entry"""
    cfg = _config()
    ws_bytes = lib.cp_online_adapt_workspace_bytes(256, 0)
    ws = 1 << 20
    raw = (ctypes.c_float * (40 * 12))()
    ms = (ctypes.c_float * 24)()
    src = (ctypes.c_int32 * 12)()
    fill = (ctypes.c_float * 12)()
    pv = (ctypes.c_int32 * 8)()
    for fn, who in ((lib.cp_online_push_mapped, b"cp_online_push_mapped"), (lib.cp_online_adapt_push_mapped, b"cp_online_adapt_push_mapped")):
        for s, f in ((src, None), (None, fill)):
            rc = fn(ctypes.byref(cfg), ws, ws_bytes, raw, 40, ms, s, f, pv, pv, None, None, None)
            assert rc == ERR_ARG and who in lib.cp_last_error() and b"go together" in lib.cp_last_error()
        rc = fn(ctypes.byref(cfg), ws, ws_bytes, None, 40, ms, None, None, pv, pv, None, None, None)      # its twin's refusals
        assert rc == ERR_ARG and who in lib.cp_last_error() and b"raw" in lib.cp_last_error()
    state = 1 << 20
    rc = lib.cp_online_windows_mapped(ctypes.byref(cfg), state, 3328, raw, 40, ms, src, None, ms, None)
    assert rc == ERR_ARG and b"cp_online_windows_mapped" in lib.cp_last_error() and b"go together" in lib.cp_last_error()
    rc = lib.cp_online_windows_mapped(ctypes.byref(cfg), state, 3327, raw, 40, ms, None, None, ms, None)
    assert rc == ERR_ARG and b"state too small" in lib.cp_last_error()


def test_map_names_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    from contrastiveprosthetics_amd import online
    for n in ("rotations", "leave_one_out", "score_channel_maps", "pick_channel_map"):
        assert getattr(pkg, n) is getattr(online, n)
