"""CPU checks of the adaptive online decoder (cp_online_adapt_*, csrc/online_adapt.cuh): the new entries are declared,
exported and bound, the workspace query, and the refusals that come before any launch."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ADAPT = ["cp_online_adapt_workspace_bytes", "cp_online_adapt_prepare", "cp_online_adapt_calibrate_scratch_bytes",
         "cp_online_adapt_calibrate", "cp_online_adapt_push", "cp_online_adapt_statistics"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def _cfg(dtype=None):
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_config()
    cfg.dtype = _lib.CP_F32 if dtype is None else dtype
    cfg.max_windows, cfg.vote, cfg.phase, cfg.n_coef = 16, 25, 0, 9
    cfg.a[0] = 1.0
    return cfg


def test_adapt_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in ADAPT:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
        assert getattr(lib, n).restype == _lib.SYMBOLS[n][0], n


def test_adapt_workspace_grows_with_windows_per_push(lib):
    from contrastiveprosthetics_amd._lib import CP_BF16, CP_F32
    for dt in (CP_F32, CP_BF16):
        sizes = [lib.cp_online_adapt_workspace_bytes(m, dt) for m in (1, 16, 17, 256)]
        assert sizes[0] == sizes[1] < sizes[2] < sizes[3], sizes                    # whole 16-row tiles
        # at least the folded workspace: cp_online_set_classes / cp_online_reset check that size on an adaptive workspace
        for m, s in zip((1, 16, 17, 256), sizes):
            assert s >= lib.cp_online_workspace_bytes(m, dt) + 9 * 2 * 512 * 8
        sc = [lib.cp_online_adapt_calibrate_scratch_bytes(n, dt) for n in (2, 256, 6000)]
        assert sc[0] < sc[1] < sc[2]
        assert sc[2] >= 6000 * (768 + 512) * (2 if dt == CP_BF16 else 4)
    assert lib.cp_online_adapt_workspace_bytes(256, CP_F32) > lib.cp_online_adapt_workspace_bytes(256, CP_BF16)


@pytest.mark.parametrize("alpha", [-0.1, 1.0, 1.5, float("nan")])
def test_alpha_outside_unit_interval_refused(lib, alpha):
    from contrastiveprosthetics_amd import _lib
    cfg, p = _cfg(), _lib.cp_params()
    buf = ctypes.create_string_buffer(1 << 12)
    assert lib.cp_online_adapt_prepare(ctypes.byref(cfg), ctypes.byref(p), None, 1e-5, alpha, buf, 1 << 12, None) == 10001
    assert b"alpha" in lib.cp_last_error()


def test_adapt_refusals_before_any_launch(lib):
    from contrastiveprosthetics_amd import _lib
    buf = ctypes.create_string_buffer(1 << 12)
    fp8 = _cfg(_lib.CP_FP8)
    p = _lib.cp_params()
    assert lib.cp_online_adapt_prepare(ctypes.byref(fp8), ctypes.byref(p), None, 1e-5, 0.01, buf, 1 << 12, None) == 10001
    assert b"dtype" in lib.cp_last_error()
    assert lib.cp_online_adapt_push(ctypes.byref(fp8), buf, 1 << 12, buf, 20, buf, buf, buf, None, None, None) == 10001
    assert b"dtype" in lib.cp_last_error()
    cfg = _cfg()
    for n in (-1, 0, 1):
        assert lib.cp_online_adapt_calibrate(ctypes.byref(cfg), buf, 1 << 12, buf, n, buf, 1 << 12, None) == 10001
        assert b"at least 2 windows" in lib.cp_last_error()
    # a workspace of the folded size is too small for the adaptive form
    small = lib.cp_online_workspace_bytes(16, _lib.CP_F32)
    assert lib.cp_online_adapt_statistics(ctypes.byref(cfg), ctypes.c_void_p(256), small, ctypes.c_void_p(256), None) == 10002


def test_python_refusals_before_any_launch(lib):
    """The decoder refuses on the host: alpha, fp8, a push before an AdaBN model is calibrated, glove rows on an AdaBN
    model and a calibration recording of fewer than 2 windows (checked without a device: the refusals come first)."""
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import OnlineDecoder, windows_before

    class _Ada:                                               # the attributes the refusals read
        adabn = True

    d = OnlineDecoder.__new__(OnlineDecoder)
    d.engine, d.adapt, d.calibrated, d.class_ids, d.phase = _Ada(), 0.01, False, object(), 0
    with pytest.raises(_lib.CpNativeError, match="calibrate"):
        d.push(None)
    with pytest.raises(_lib.CpNativeError, match="AdaBN"):
        d.set_classes(glove=[[0.0] * 20])
    n1 = max(n for n in range(200) if windows_before(n) == 1)     # the longest recording of one window

    class _Raw:
        def dim(self):
            return 2
        shape = (n1, 12)
    with pytest.raises(ValueError, match="at least 2 windows"):
        d.calibrate(_Raw())
    d.adapt = None
    with pytest.raises(_lib.CpNativeError, match="adaptive form"):
        d.calibrate(_Raw())
    e = type("E", (), {"adabn": False})()
    try:
        import contrastiveprosthetics_amd.online as online
        orig = online._engine_of
        online._engine_of = lambda m: m
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            OnlineDecoder(e, 0.0, 1.0, adapt=1.0)
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            OnlineDecoder(e, 0.0, 1.0, adapt=-0.5)
        with pytest.raises(_lib.CpNativeError, match="AdaBN"):
            OnlineDecoder(_Ada(), 0.0, 1.0)
        with pytest.raises(_lib.CpNativeError, match="8-bit"):
            OnlineDecoder(_Ada(), 0.0, 1.0, dtype="fp8", adapt=0.01)
    finally:
        online._engine_of = orig
