"""CPU checks of the adaptive multi-stream online decoder (contrastiveprosthetics_amd/online.py AdaptiveMultiStreamDecoder,
csrc/online_multi_adapt.cuh): the C ABI of the cp_online_multi_adapt_* entries, the workspace query and argument refusals
before any device call."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ADAPT = ["cp_online_multi_adapt_workspace_bytes", "cp_online_multi_adapt_prepare", "cp_online_multi_adapt_set_alpha",
         "cp_online_multi_adapt_reset_statistics", "cp_online_multi_adapt_calibrate", "cp_online_multi_adapt_push",
         "cp_online_multi_adapt_statistics"]
ERR_ARG, ERR_WORKSPACE = 10001, 10002
STATS_BYTES = 9 * 2 * 512 * 8


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_multi_adapt_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in ADAPT:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    assert int(re.search(r"#define CP_VERSION (\d+)", open(HEADER).read()).group(1)) == 112
    assert lib.cp_version() == 112


def test_multi_adapt_workspace_grows_and_counts_the_weights_once(lib):
    from contrastiveprosthetics_amd._lib import CP_BF16, CP_F32
    for dt in (CP_F32, CP_BF16):
        ws = lib.cp_online_multi_adapt_workspace_bytes
        rows = [ws(4, r, dt) for r in (1, 16, 17, 256, 4096)]
        assert rows[0] == rows[1] < rows[2] < rows[3] < rows[4], rows                 # whole 16-row tiles
        streams = [ws(s, 64, dt) for s in (1, 2, 64, 256)]
        assert streams[0] < streams[1] < streams[2] < streams[3], streams
        single = lib.cp_online_adapt_workspace_bytes(1, dt)
        assert ws(64, 64, dt) < 64 * single / 10, (ws(64, 64, dt), single)
        per_stream = (ws(256, 64, dt) - ws(1, 64, dt)) / 255
        assert STATS_BYTES <= per_stream < 96 * 1024, per_stream                       # its state and 72 KiB of statistics
        # the workspace begins as a cp_online_multi_* one, which the shared set_classes / reset entries check
        assert ws(7, 100, dt) >= lib.cp_online_multi_workspace_bytes(7, 100, dt)
        assert ws(1, 256, dt) >= lib.cp_online_adapt_workspace_bytes(256, dt) - 2 * 256


def _cfg():
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_config()
    cfg.dtype, cfg.max_windows, cfg.vote, cfg.phase, cfg.n_coef = _lib.CP_F32, 16, 25, 0, 9
    cfg.a[0] = 1.0
    return cfg


def test_multi_adapt_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory as the 'workspace': every refusal returns before a launch, which on this machine would fail differently"""
    from contrastiveprosthetics_amd import _lib
    S, R = 4, 32
    cfg = _cfg()
    need = lib.cp_online_multi_adapt_workspace_bytes(S, R, cfg.dtype)
    buf = ctypes.create_string_buffer(need + 256)
    ws = (ctypes.addressof(buf) + 255) // 256 * 256
    cr = ctypes.byref(cfg)

    def err(rc, what):
        assert rc == ERR_ARG, (rc, what)
        assert what.encode() in lib.cp_last_error(), (what, lib.cp_last_error())

    out = (ctypes.c_double * (9 * 2 * 512))()
    # n_streams, max_rows, workspace
    err(lib.cp_online_multi_adapt_statistics(cr, 0, R, ws, need, 0, out, None), "n_streams")
    err(lib.cp_online_multi_adapt_statistics(cr, 257, R, ws, need, 0, out, None), "n_streams")
    err(lib.cp_online_multi_adapt_statistics(cr, S, 0, ws, need, 0, out, None), "max_rows")
    err(lib.cp_online_multi_adapt_statistics(cr, S, 65537, ws, need, 0, out, None), "max_rows")
    err(lib.cp_online_multi_adapt_statistics(cr, S, R, None, need, 0, out, None), "workspace")
    assert lib.cp_online_multi_adapt_statistics(cr, S, R, ws, need - 1, 0, out, None) == ERR_WORKSPACE
    assert lib.cp_online_multi_adapt_statistics(cr, S, R + 16, ws, need, 0, out, None) == ERR_WORKSPACE
    assert lib.cp_online_multi_adapt_statistics(cr, S + 1, R, ws, need, 0, out, None) == ERR_WORKSPACE
    # stream index
    for idx in (S, -1):
        err(lib.cp_online_multi_adapt_statistics(cr, S, R, ws, need, idx, out, None), "stream index")
        err(lib.cp_online_multi_adapt_set_alpha(cr, S, R, ws, need, idx, 0.1, None), "stream index")
        err(lib.cp_online_multi_adapt_reset_statistics(cr, S, R, ws, need, idx, None, None), "stream index")
    err(lib.cp_online_multi_adapt_statistics(cr, S, R, ws, need, 0, None, None), "out")
    # alpha outside [0, 1)
    for a in (-1e-9, 1.0, 2.0, float("nan")):
        err(lib.cp_online_multi_adapt_set_alpha(cr, S, R, ws, need, 0, a, None), "alpha")
    # calibration: fewer than 2 windows, index, scratch
    win = (ctypes.c_float * (12 * 4))()
    sb = lib.cp_online_adapt_calibrate_scratch_bytes(4, cfg.dtype)
    sbuf = ctypes.create_string_buffer(sb + 256)
    sc = (ctypes.addressof(sbuf) + 255) // 256 * 256
    err(lib.cp_online_multi_adapt_calibrate(cr, S, R, ws, need, 0, win, 1, sc, sb, None), "at least 2 windows")
    err(lib.cp_online_multi_adapt_calibrate(cr, S, R, ws, need, S, win, 4, sc, sb, None), "stream index")
    err(lib.cp_online_multi_adapt_calibrate(cr, S, R, ws, need, 0, win, 4, None, sb, None), "scratch")
    assert lib.cp_online_multi_adapt_calibrate(cr, S, R, ws, need, 0, win, 4, sc, sb - 1, None) == ERR_WORKSPACE
    # push: total_windows, counts, pred / voted
    raw = (ctypes.c_float * 12)()
    cnt = (ctypes.c_int32 * S)()
    ms = (ctypes.c_float * 24)()
    pv = (ctypes.c_int32 * (R + 1))()
    P = lib.cp_online_multi_adapt_push
    err(P(cr, S, R, ws, need, raw, cnt, 1, R + 1, ms, pv, pv, None, None, None), "total_windows")
    err(P(cr, S, R, ws, need, raw, cnt, -1, 0, ms, pv, pv, None, None, None), "total_samples")
    err(P(cr, S, R, ws, need, raw, None, 1, 0, ms, pv, pv, None, None, None), "counts")
    err(P(cr, S, R, ws, need, raw, cnt, 20, 1, ms, None, pv, None, None, None), "pred")
    err(P(cr, S, R, ws, need, raw, cnt, 20, 1, ms, pv, None, None, None, None), "pred")
    assert P(cr, S, R, ws, need, None, None, 0, 0, None, None, None, None, None, None) == 0      # nothing to do
    # prepare: parameters, eps
    p = _lib.cp_params()
    err(lib.cp_online_multi_adapt_prepare(cr, S, R, ctypes.byref(p), None, 1e-5, None, ws, need, None), "parameters")
    err(lib.cp_online_multi_adapt_prepare(cr, S, R, ctypes.byref(p), None, 0.0, None, ws, need, None), "bn_eps")
    for a in (-1e-9, 1.0, float("nan")):                                             # alpha outside [0, 1), for any stream
        alphas = (ctypes.c_double * S)(0.1, 0.0, a, 0.5)
        err(lib.cp_online_multi_adapt_prepare(cr, S, R, ctypes.byref(p), None, 1e-5, alphas, ws, need, None), "alpha")
    # fp8: no 8-bit path, in every entry
    cfg.dtype = 2
    err(lib.cp_online_multi_adapt_statistics(cr, S, R, ws, need, 0, out, None), "8-bit")
    err(lib.cp_online_multi_adapt_set_alpha(cr, S, R, ws, need, 0, 0.1, None), "8-bit")
    err(P(cr, S, R, ws, need, raw, cnt, 20, 1, ms, pv, pv, None, None, None), "8-bit")
    err(lib.cp_online_multi_adapt_calibrate(cr, S, R, ws, need, 0, win, 4, sc, sb, None), "8-bit")
    err(lib.cp_online_multi_adapt_reset_statistics(cr, S, R, ws, need, 0, None, None), "8-bit")


def test_adaptive_multi_decoder_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder
    assert pkg.AdaptiveMultiStreamDecoder is AdaptiveMultiStreamDecoder
