"""CPU checks of the per-stream projections of the multi-stream decoders (include/cpnative.h "per-stream projections",
csrc/online_projections.cuh, online.py `stream_projections=True`): the size of a bank, the workspace totals it must not move, the
header against the binding, the refusals of every new C entry before anything is enqueued, and the refusals of the Python layer
on decoders that have no device behind them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
HEADER = os.path.join(ROOT, "include", "cpnative.h")
ERR_ARG, ERR_WORKSPACE = 10001, 10002
NEW = ["cp_online_projections_bytes", "cp_online_projections_set", "cp_online_projections_get", "cp_online_projections_clear",
       "cp_online_multi_push_proj", "cp_online_multi_adapt_push_proj", "cp_online_multi_enroll_proj",
       "cp_online_multi_adapt_enroll_proj", "cp_online_multi_map_sweep_proj", "cp_online_multi_adapt_map_sweep_proj"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------------------------
def test_bank_bytes_follow_the_documented_formula(lib):
    from contrastiveprosthetics_amd._lib import CP_BF16, CP_F32
    for dt, es in ((CP_F32, 4), (CP_BF16, 2)):
        for n in (1, 3, 256):
            assert lib.cp_online_projections_bytes(n, dt) == n * (16 * 512 * es + 256)
        sizes = [lib.cp_online_projections_bytes(n, dt) for n in range(1, 257)]
        assert all(s % 256 == 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
        assert lib.cp_online_projections_bytes(0, dt) == sizes[0]          # as the other size queries: at least one stream


def test_the_workspace_totals_have_not_moved(lib):
    """the bank is a buffer of its own: the totals tests/test_online_workspace_host.py pins for the two multi-stream forms"""
    from contrastiveprosthetics_amd._lib import CP_BF16, CP_F32
    pairs = [(1, 1), (3, 17), (7, 100), (256, 4096), (256, 65536)]
    want = {"cp_online_multi_workspace_bytes": ([8055552, 8153600, 8597760, 31101184, 348623104],
                                                [4041472, 4098560, 4337920, 16642304, 176877824]),
            "cp_online_multi_adapt_workspace_bytes": ([8360192, 8802304, 10524416, 100345344, 1172841984],
                                                      [4272384, 4599808, 5748480, 67012096, 699106816])}
    for entry, per_dtype in want.items():
        for dt, totals in zip((CP_F32, CP_BF16), per_dtype):
            assert [getattr(lib, entry)(s, r, dt) for s, r in pairs] == totals, (entry, dt)


# ---------------------------------------------------------------------------------------------------------------------------
# header and binding
# ---------------------------------------------------------------------------------------------------------------------------
_CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int}


def _header_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^(int|size_t)\s+(cp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        if name not in NEW:
            continue
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            if "*" in a:
                types.append("cfg" if a.startswith("const cp_online_config*") else "ptr")
            else:
                types.append(_CTYPE[a.split()[-2]])
        out[name] = (_CTYPE[ret], types)
    return out


def test_header_prototypes_equal_the_binding(lib):
    from contrastiveprosthetics_amd import _lib
    protos = _header_prototypes()
    raw = C.CDLL(LIB)
    for name in NEW:
        assert name in protos, f"{name} is not declared in cpnative.h"
        assert hasattr(raw, name), f"{name} is not exported"
        res, args = _lib.SYMBOLS[name]
        want_res, want_args = protos[name]
        assert res == want_res, name
        got = ["cfg" if a == C.POINTER(_lib.cp_online_config) else "ptr" if a == C.c_void_p else a for a in args]
        assert got == want_args, (name, got, want_args)
    # every prototype cites what it belongs to: the block names the entries it extends
    block = open(HEADER).read().split("per-stream projections: each stream", 1)[1]
    for cited in ("cp_online_multi_push_embed", "cp_online_multi_adapt_push_embed", "cp_online_multi_enroll",
                  "cp_online_multi_adapt_enroll", "cp_online_multi_map_sweep", "cp_online_multi_adapt_map_sweep", "set_projection"):
        assert cited in block, cited


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries refuse before anything is enqueued (no device is touched: every pointer below is a made-up address)
# ---------------------------------------------------------------------------------------------------------------------------
FAKE = 0x7F0000000000                          # 256-byte aligned; never dereferenced by a refused call
S, ROWS = 3, 17


def _cfg(dtype="f32"):
    from contrastiveprosthetics_amd import online
    b, a = online._filter(None, None)
    return online._config(dtype, 256, 25, 0, b, a)


def _refused(lib, rc, code, who, what):
    msg = lib.cp_last_error().decode()
    assert rc == code, (who, rc, msg)
    assert who in msg and what in msg, msg


def test_bank_entries_refuse_bad_arguments(lib):
    from contrastiveprosthetics_amd._lib import CP_F32, CP_FP8
    need = lib.cp_online_projections_bytes(S, CP_F32)
    P = FAKE + (1 << 20)
    calls = {
        "cp_online_projections_set": lambda dt, bank, nbytes, n, i: lib.cp_online_projections_set(dt, bank, nbytes, n, i, P, P, None),
        "cp_online_projections_get": lambda dt, bank, nbytes, n, i: lib.cp_online_projections_get(dt, bank, nbytes, n, i, P, P, None, None),
        "cp_online_projections_clear": lambda dt, bank, nbytes, n, i: lib.cp_online_projections_clear(dt, bank, nbytes, n, i, None),
    }
    for who, call in calls.items():
        _refused(lib, call(CP_F32, None, need, S, 0), ERR_ARG, who, "bank is required")
        _refused(lib, call(CP_F32, FAKE + 16, need, S, 0), ERR_ARG, who, "256-byte aligned")
        _refused(lib, call(CP_F32, FAKE, need - 1, S, 0), ERR_WORKSPACE, who, "bank too small")
        _refused(lib, call(CP_F32, FAKE, 0, S, 0), ERR_WORKSPACE, who, "bank too small")
        _refused(lib, call(CP_FP8, FAKE, need, S, 0), ERR_ARG, who, "dtype")
        _refused(lib, call(7, FAKE, need, S, 0), ERR_ARG, who, "dtype")
        _refused(lib, call(CP_F32, FAKE, need, 0, 0), ERR_ARG, who, "n_streams")
        _refused(lib, call(CP_F32, FAKE, need * 100, 257, 0), ERR_ARG, who, "n_streams")
        _refused(lib, call(CP_F32, FAKE, need, S, S), ERR_ARG, who, "stream index")
        _refused(lib, call(CP_F32, FAKE, need, S, -2), ERR_ARG, who, "stream index")
    for who in ("cp_online_projections_set", "cp_online_projections_get"):       # -1 (all) is clear's alone
        _refused(lib, calls[who](CP_F32, FAKE, need, S, -1), ERR_ARG, who, "stream index")
    _refused(lib, lib.cp_online_projections_set(CP_F32, FAKE, need, S, 0, None, P, None), ERR_ARG, "cp_online_projections_set", "W and b")
    _refused(lib, lib.cp_online_projections_get(CP_F32, FAKE, need, S, 0, P, None, None, None), ERR_ARG, "cp_online_projections_get",
             "W and b")


@pytest.mark.parametrize("adaptive", [False, True])
def test_proj_entries_refuse_a_bad_bank_index_or_dtype(lib, adaptive):
    from contrastiveprosthetics_amd._lib import CP_F32
    form = "cp_online_multi_adapt" if adaptive else "cp_online_multi"
    cfg = _cfg()
    ws_bytes = getattr(lib, form + "_workspace_bytes")(S, ROWS, CP_F32)
    need = lib.cp_online_projections_bytes(S, CP_F32)
    head = (C.byref(cfg), S, ROWS, FAKE, ws_bytes)
    P = FAKE + (1 << 30)

    def push(bank, nbytes, c=cfg):
        return getattr(lib, form + "_push_proj")(C.byref(c), S, ROWS, FAKE, ws_bytes, P, P, 100, 5, P, None, None, P, P, None, None, None,
                                                 bank, nbytes, None)

    def enroll(index, bank, nbytes, c=cfg):
        return getattr(lib, form + "_enroll_proj")(C.byref(c), S, ROWS, FAKE, ws_bytes, index, bank, nbytes, P, 10, P, 4, P, P, 1 << 30, None)

    def sweep(index, bank, nbytes, c=cfg):
        return getattr(lib, form + "_map_sweep_proj")(C.byref(c), S, ROWS, FAKE, ws_bytes, index, bank, nbytes, P, 10, P, P, P, 2, 4, P, 0, P,
                                                      1 << 30, P, None, P, None, None)

    bank2 = FAKE + (1 << 31)
    for who, call in ((form + "_push_proj", push), (form + "_enroll_proj", lambda *a, **k: enroll(0, *a, **k)),
                      (form + "_map_sweep_proj", lambda *a, **k: sweep(0, *a, **k))):
        _refused(lib, call(bank2, need - 1), ERR_WORKSPACE, who, "bank too small")
        _refused(lib, call(bank2, 0), ERR_WORKSPACE, who, "bank too small")
        _refused(lib, call(bank2 + 64, need), ERR_ARG, who, "256-byte aligned")
        bad = _cfg()
        bad.dtype = 2                                           # CP_FP8: no 8-bit online path, with or without a bank
        _refused(lib, call(bank2, need, c=bad), ERR_ARG, "cp_online", "dtype")
        # a bank sized for bf16 under an f32 configuration is short
        _refused(lib, call(bank2, lib.cp_online_projections_bytes(S, 1)), ERR_WORKSPACE, who, "bank too small")
    for who, call in ((form + "_enroll_proj", enroll), (form + "_map_sweep_proj", sweep)):
        for index in (-1, S, 256):
            _refused(lib, call(index, bank2, need), ERR_ARG, who, "stream index")
            _refused(lib, call(index, None, 0), ERR_ARG, who, "stream index")        # also without a bank
    # a workspace that is too small is refused in the form's own words, before the bank is looked at
    rc = getattr(lib, form + "_push_proj")(*head[:4], ws_bytes - 1, P, P, 100, 5, P, None, None, P, P, None, None, None, bank2, 0, None)
    _refused(lib, rc, ERR_WORKSPACE, form, "workspace too small")
    assert head[3] == FAKE


# ---------------------------------------------------------------------------------------------------------------------------
# the Python layer on decoders without a device
# ---------------------------------------------------------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"a refused call reached the library entry {name}")


def _stub(cls, on: bool, n_streams: int = 4):
    d = cls.__new__(cls)
    d.n_streams, d.device, d.lib, d.phase = n_streams, "cpu", _NoDevice(), 0
    d.class_ids = [None] * n_streams
    d.stream_projections = on
    d._bank = _NoDevice() if on else None
    if on:
        d._shared_projection = False
        d._own_projection = np.zeros(n_streams, dtype=bool)
    return d


@pytest.mark.parametrize("form", ["MultiStreamDecoder", "AdaptiveMultiStreamDecoder"])
def test_python_refusals_with_the_option_off_are_todays(form):
    from contrastiveprosthetics_amd import _lib, online, readout
    import inspect
    cls = getattr(online, form)
    assert cls._shared_projection is True
    assert inspect.signature(cls.__init__).parameters["stream_projections"].default is False
    d = _stub(cls, False)
    assert d._shared_projection and not d.has_projection(0)
    with pytest.raises(ValueError, match="shared by all streams"):
        d.finetune(0, torch.zeros(100, 12), np.zeros(100), train_projection=True)
    W, b = np.zeros((16, 512), np.float32), np.zeros(16, np.float32)
    with pytest.raises(_lib.CpNativeError, match="share one projection.*stream_projections=True"):
        d.set_projection(0, W, b)
    with pytest.raises(_lib.CpNativeError, match="stream_projections=True"):
        d.reset_projection()
    fit = readout.Readout(W[None], b[None], [0], [((0,), 0.1)], {2: 30}, [2], "f32")
    for kw in ({}, {"stream": 0}):
        with pytest.raises(_lib.CpNativeError, match="share one projection"):
            fit.install(d, 0, **kw)


@pytest.mark.parametrize("form", ["MultiStreamDecoder", "AdaptiveMultiStreamDecoder"])
def test_python_refusals_with_the_option_on_come_before_any_device_call(form):
    from contrastiveprosthetics_amd import _lib, online, readout
    d = _stub(getattr(online, form), True)
    assert not d._shared_projection and type(d)._shared_projection
    W, b = np.zeros((16, 512), np.float32), np.zeros(16, np.float32)
    for bad in (-1, 4, 1.0, True, None, "0"):
        with pytest.raises(IndexError):
            d.set_projection(bad, W, b)
        with pytest.raises(IndexError):
            d.has_projection(bad)
        with pytest.raises(IndexError):
            d.projection(bad)
    for bad in (4, -1, 1.5):
        with pytest.raises(IndexError):
            d.reset_projection(bad)
    for Wb, bb in ((W[:15], b), (W[:, :511], b), (W.T, b), (W, b[:15]), (W, b[None]), (W.reshape(-1), b), (np.float32(0), b)):
        with pytest.raises(ValueError, match=r"\(16, 512\)"):
            d.set_projection(0, Wb, bb)
    for value in (np.nan, np.inf, -np.inf):
        Wn, bn = W.copy(), b.copy()
        Wn[7, 300] = value
        bn[15] = value
        with pytest.raises(ValueError, match="finite"):
            d.set_projection(0, Wn, b)
        with pytest.raises(ValueError, match="finite"):
            d.set_projection(0, torch.from_numpy(W), torch.from_numpy(bn))
    assert not d._own_projection.any()
    # a readout: the plan and the stream are checked before the decoder is asked for anything
    fit = readout.Readout(np.zeros((2, 16, 512), np.float32), np.zeros((2, 16), np.float32), [0, 7], [((0,), 0.1), ((0,), 0.0)], {2: 30},
                          [2], "f32")
    with pytest.raises(IndexError):
        fit.install(d, 0, stream=4)
    with pytest.raises(ValueError, match="positive definite"):
        fit.install(d, 1, stream=0)
    with pytest.raises(_lib.CpNativeError, match="share one projection"):
        fit.install(d, 0)                                       # a multi-stream decoder without stream=

    class Single:
        class_ids = None

        def set_projection(self, W, b):
            raise AssertionError("never installed")

    with pytest.raises(ValueError, match="stream= goes with a multi-stream decoder"):
        fit.install(Single(), 0, stream=0)
