"""CPU checks of the multi-stream online decoder (contrastiveprosthetics_amd/online.py MultiStreamDecoder, csrc/online_multi.cuh):
the C ABI of the cp_online_multi_* entries, the workspace query, argument refusals before any device call, and the host's
packing and splitting of a push."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
MULTI = ["cp_online_multi_workspace_bytes", "cp_online_multi_prepare", "cp_online_multi_set_classes", "cp_online_multi_reset",
         "cp_online_multi_push"]
ERR_ARG, ERR_WORKSPACE = 10001, 10002


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_multi_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in MULTI:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    for name in ("MAX_STREAMS", "MAX_ROWS"):
        v = int(re.search(r"#define CP_ONLINE_MULTI_%s (\d+)" % name, hdr).group(1))
        assert getattr(_lib, "CP_ONLINE_MULTI_" + name) == v, name
    assert int(re.search(r"#define CP_VERSION (\d+)", open(HEADER).read()).group(1)) == 112


def test_multi_workspace_grows_with_streams_and_rows_and_shares_the_weights(lib):
    from contrastiveprosthetics_amd._lib import CP_BF16, CP_F32
    for dt in (CP_F32, CP_BF16):
        ws = lib.cp_online_multi_workspace_bytes
        rows = [ws(4, r, dt) for r in (1, 16, 17, 256, 4096)]
        assert rows[0] == rows[1] < rows[2] < rows[3] < rows[4], rows                 # whole 16-row tiles
        streams = [ws(s, 64, dt) for s in (1, 2, 64, 256)]
        assert streams[0] < streams[1] < streams[2] < streams[3], streams
        single = lib.cp_online_workspace_bytes(1, dt)
        assert single > 4 * 1000 * 1000 // (2 if dt == CP_BF16 else 1)               # mostly the folded weights
        # the weights are counted once: 64 streams x 1 window cost a small fraction of 64 single-stream workspaces
        assert ws(64, 64, dt) < 64 * single / 20, (ws(64, 64, dt), single)
        assert ws(64, 64, dt) - ws(1, 64, dt) < 63 * 16 * 1024                         # per stream: its state, not weights
        assert ws(1, 256, dt) >= lib.cp_online_workspace_bytes(256, dt)
    assert lib.cp_online_multi_workspace_bytes(64, 256, CP_F32) > lib.cp_online_multi_workspace_bytes(64, 256, CP_BF16)


def _cfg():
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_config()
    cfg.dtype, cfg.max_windows, cfg.vote, cfg.phase, cfg.n_coef = _lib.CP_F32, 16, 25, 0, 9
    cfg.a[0] = 1.0
    return cfg


def test_multi_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory as the 'workspace': every refusal returns before a launch, which on this machine would fail differently"""
    S, R = 4, 32
    cfg = _cfg()
    need = lib.cp_online_multi_workspace_bytes(S, R, cfg.dtype)
    buf = ctypes.create_string_buffer(need + 256)
    ws = (ctypes.addressof(buf) + 255) // 256 * 256
    tab = (ctypes.c_float * 16)()
    ids = (ctypes.c_int32 * 1)()
    cr = ctypes.byref(cfg)

    def err(rc, what):
        assert rc == ERR_ARG, rc
        assert what.encode() in lib.cp_last_error(), lib.cp_last_error()

    err(lib.cp_online_multi_reset(cr, S, R, None, need, 0, None), "workspace")
    err(lib.cp_online_multi_reset(cr, 0, R, ws, need, 0, None), "n_streams")
    err(lib.cp_online_multi_reset(cr, 257, R, ws, need, 0, None), "n_streams")
    err(lib.cp_online_multi_reset(cr, S, 0, ws, need, 0, None), "max_rows")
    err(lib.cp_online_multi_reset(cr, S, 65537, ws, need, 0, None), "max_rows")
    err(lib.cp_online_multi_reset(cr, S, R, ws, need, S, None), "stream index")
    err(lib.cp_online_multi_reset(cr, S, R, ws, need, -2, None), "stream index")
    err(lib.cp_online_multi_set_classes(cr, S, R, ws, need, S, tab, ids, 1, None), "stream index")
    err(lib.cp_online_multi_set_classes(cr, S, R, ws, need, -1, tab, ids, 1, None), "stream index")
    err(lib.cp_online_multi_set_classes(cr, S, R, ws, need, 0, tab, ids, 65, None), "classes")
    assert lib.cp_online_multi_reset(cr, S, R, ws, need - 1, 0, None) == ERR_WORKSPACE
    assert lib.cp_online_multi_reset(cr, S, R + 16, ws, need, 0, None) == ERR_WORKSPACE     # sized for fewer rows
    raw = (ctypes.c_float * 12)()
    cnt = (ctypes.c_int32 * S)()
    ms = (ctypes.c_float * 24)()
    pv = (ctypes.c_int32 * (R + 1))()
    err(lib.cp_online_multi_push(cr, S, R, ws, need, raw, cnt, 1, R + 1, ms, pv, pv, None, None, None), "total_windows")
    err(lib.cp_online_multi_push(cr, S, R, ws, need, raw, cnt, -1, 0, ms, pv, pv, None, None, None), "total_samples")
    err(lib.cp_online_multi_push(cr, S, R, ws, need, raw, None, 1, 0, ms, pv, pv, None, None, None), "counts")
    err(lib.cp_online_multi_push(cr, S, R, ws, need, raw, cnt, 20, 1, ms, None, pv, None, None, None), "pred")
    assert lib.cp_online_multi_push(cr, S, R, ws, need, None, None, 0, 0, None, None, None, None, None, None) == 0   # nothing to do
    cfg.dtype = 2                                                                   # fp8: no 8-bit online path
    err(lib.cp_online_multi_reset(cr, S, R, ws, need, 0, None), "dtype")
    from contrastiveprosthetics_amd import _lib
    p = _lib.cp_params()
    cfg.dtype = _lib.CP_F32
    assert lib.cp_online_multi_prepare(cr, S, R, ctypes.byref(p), None, 1e-5, ws, need, None) == ERR_ARG     # AdaBN / no params


def test_packed_rows_agree_with_windows_emitted_per_stream():
    """For random chunkings of S independent streams: the rows the host packs each stream into are windows_emitted of that
    stream's own count, in stream order, and a stream's windows over all pushes are those of the stream pushed alone."""
    from contrastiveprosthetics_amd.online import packed_rows, windows_before, windows_emitted
    rng = np.random.default_rng(3)
    for phase in (0, 7, 19):
        S = 9
        seen = np.zeros(S, dtype=np.int64)
        total = np.zeros(S, dtype=np.int64)
        for _ in range(60):
            counts = rng.integers(0, 90, S) * (rng.random(S) < 0.6)
            row0, m = packed_rows(seen, counts, phase)
            assert list(m) == [windows_emitted(int(seen[s]), int(counts[s]), phase) for s in range(S)]
            assert row0[0] == 0 and all(row0[s + 1] == row0[s] + m[s] for s in range(S - 1))
            seen += counts
            total += m
        assert list(total) == [windows_before(int(n), phase) for n in seen]


def test_plan_splits_pushes_in_order_within_the_caps():
    from contrastiveprosthetics_amd.online import packed_rows, plan_push, windows_before
    rng = np.random.default_rng(4)
    for _ in range(400):
        S = int(rng.integers(1, 40))
        seen = rng.integers(0, 3000, S)
        counts = rng.integers(0, 2000, S) * (rng.random(S) < 0.7)
        W, R, phase = int(rng.integers(1, 30)), int(rng.integers(1, 80)), int(rng.integers(0, 20))
        rounds = plan_push(seen, counts, phase, W, R)
        assert np.array_equal(np.sum(rounds, axis=0) if rounds else np.zeros(S), counts)
        s = seen.copy()
        for take in rounds:
            assert take.sum() > 0 and (take >= 0).all()
            _, m = packed_rows(s, take, phase)
            assert m.max() <= W and m.sum() <= R
            s = s + take
        assert all(windows_before(int(a), phase) - windows_before(int(b), phase) >= 0 for a, b in zip(s, seen))
    # what fits is one round
    assert len(plan_push([0] * 64, [20] * 64, 0, 256, 64)) == 1
    assert len(plan_push([0] * 64, [20] * 64, 0, 256, 63)) == 2


def test_multi_decoder_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    from contrastiveprosthetics_amd.online import MultiStreamDecoder
    assert pkg.MultiStreamDecoder is MultiStreamDecoder
