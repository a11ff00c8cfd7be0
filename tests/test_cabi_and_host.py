"""CPU-only checks: the C-ABI library loads and exports every symbol include/cpnative.h declares
(no compute call is made -- there is no GPU here), and the host-side logic (constants, parameter
table, CLI surface, sharding) matches the oracle / the reference's published layout."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_bound_and_at_version_112(lib):
    """every function include/cpnative.h declares is exported and has a ctypes prototype, nothing else is bound, and the library
    reports the header's CP_VERSION (112: cp_config.record), which is also the binding's minimum"""
    from contrastiveprosthetics_amd import _lib
    names = declared_functions()
    assert len(names) >= 15
    raw = ctypes.CDLL(LIB)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in cpnative.h but not exported"
        assert n in _lib.SYMBOLS, f"{n} has no ctypes prototype in _lib.SYMBOLS"
    assert set(_lib.SYMBOLS) == set(names)
    version = int(re.search(r"#define CP_VERSION (\d+)", open(HEADER).read()).group(1))
    assert lib.cp_version() == version == 112
    assert f"lib.cp_version() < {version}:" in open(os.path.join(ROOT, "contrastiveprosthetics_amd", "_lib.py")).read()


def test_struct_layouts_match_header_with_forward_record():
    from contrastiveprosthetics_amd import _lib
    assert ctypes.sizeof(_lib.cp_params) == 8 * (4 + 7 + 7 + 9 + 9 + 3)
    assert ctypes.sizeof(_lib.cp_bn_buffers) == 8 * 18
    # 56 bytes of round 1-3 fields + options, tile_schedule, the sync-BN hook (fn, user, world, pad), the gradient tap (ptr, bytes),
    # the second stream (stream, fork, join) and the forward record
    assert ctypes.sizeof(_lib.cp_config) == (8 + 4 * 4 + 4 * 4 + 8 + 8) + 4 + 4 + 8 + 8 + 4 + 4 + 8 + 8 + 3 * 8 + 8
    assert ctypes.sizeof(_lib.cp_forward_record) == 8 + 4 * 4 + 8
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert ctypes.sizeof(_lib.cp_debug_fc_gemm_args) == 8 + 8 + 4 * 4 + 7 * 8 + 4 * 4 + 8
    for struct in ("cp_config", "cp_forward_record", "cp_debug_fc_gemm_args"):
        body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
        fields = re.findall(r"\b(\w+)\s*;", body)
        assert fields == [f[0] for f in getattr(_lib, struct)._fields_], fields
    for name, bit in _lib.OPTIONS.items():
        assert re.search(r"#define CP_OPT_%s %du\b" % (name.upper(), bit), open(HEADER).read()), name
    assert ctypes.sizeof(_lib.cp_adam_hyper) == 32


def test_host_only_entry_points(lib):
    # pure host functions: workspace sizing and argument validation (return before touching a device)
    small = lib.cp_workspace_bytes(41 * 8, 0, 0.0)
    big = lib.cp_workspace_bytes(41 * 4096, 1, 0.0635)
    assert 0 < small < big < 8 * 2 ** 30
    assert lib.cp_workspace_bytes(0, 0, 0.0) == 0
    assert lib.cp_workspace_bytes(41 * 4096, 1, 0.0635) > lib.cp_workspace_bytes(41 * 4096, 1, 0.0)
    rc = lib.cp_gather_groups(None, 0, None, 0, None, 0, 1, None, None)
    assert rc == 10001 and b"cp_gather_groups" in lib.cp_last_error()
    numel = (ctypes.c_int64 * 3)(5000, 64, 1)
    assert lib.cp_optimizer_scratch_floats(numel, 3) >= 3 + 1 + 1


def test_preprocess_entry_validates_long_segments_before_it_launches(lib):
    """cp_preprocess_emg checks its keep list against the RMS series in 32 bits, at a segment length a 16-bit position
    cannot hold: every refusal returns before a launch (the device pointers are dummies)"""
    seg_len, win = 70000, 11
    n_rms = seg_len - 2 * (win // 2)
    b = (ctypes.c_double * 9)(*([0.1] * 9))
    a = (ctypes.c_double * 9)(1.0, *([0.0] * 8))
    dummy = ctypes.create_string_buffer(64)

    def call(idx, n_out=None, length=seg_len):
        t = (ctypes.c_int32 * len(idx))(*idx)
        return lib.cp_preprocess_emg(dummy, 1, length, b, a, 9, win, 1024.0, t, len(idx) if n_out is None else n_out, dummy, None)

    for name, rc in (("time_idx = [n_rms]", call([n_rms])),
                     ("time_idx = [0, n_rms - 1, n_rms]", call([0, n_rms - 1, n_rms])),
                     ("time_idx = [-1]", call([-1])),
                     ("time_idx = [65536 + n_rms]", call([65536 + n_rms])),       # in range once truncated to 16 bits
                     ("n_out = 257", call([0] * 257)),
                     ("n_out = 0", call([0], n_out=0)),
                     ("seg_len < rms_window", call([0], length=win - 1))):
        assert rc == 10001, (name, rc, lib.cp_last_error())
        assert b"cp_preprocess_emg" in lib.cp_last_error(), name


def test_glove_entries_refuse_misaligned_pointers_before_they_launch(lib):
    """cp_glove_forward reads `glove` and stores `zg` in 16-byte pieces, cp_head_glove reads `z` and `zg` so: a pointer 4 bytes
    off is refused with CP_ERR_ARG and a message that names the entry and the argument, before any launch (every pointer is
    a dummy address that is never dereferenced; sizes and workspaces are valid, so the alignment check is what refuses)"""
    from contrastiveprosthetics_amd import _lib
    B, T = 3, 41
    rows = B * T
    ok, ws, gws = 0x100000, 0x200000, 0x40000000                  # 256-byte aligned addresses
    for dtype in (0, 1):                                          # CP_F32, CP_BF16
        cfg = _lib.cp_config()
        cfg.n_windows, cfg.dtype, cfg.training, cfg.bn_momentum, cfg.bn_eps = rows, dtype, 1, 0.1, 1e-5
        nb, gnb = lib.cp_workspace_bytes(rows, dtype, 0.0), lib.cp_glove_workspace_bytes(rows, dtype)
        assert nb > 0 and gnb > 0
        gp = _lib.cp_glove_params(ok, ok, ok, ok, ok, ok)

        def forward(glove, zg):
            return lib.cp_glove_forward(ctypes.byref(cfg), ctypes.byref(gp), glove, rows, gws, gnb, zg, None)

        def head(z, zg):
            return lib.cp_head_glove(ctypes.byref(cfg), z, zg, ok, B, 1, 1, ws, nb, gws, gnb, ok, ok, None, None)

        for entry, arg, call, ptrs in (("cp_glove_forward", "glove", forward, (ok + 4, ok)),
                                       ("cp_glove_forward", "zg", forward, (ok, ok + 4)),
                                       ("cp_glove_forward", "glove", forward, (ok + 8, ok + 8)),
                                       ("cp_head_glove", "z", head, (ok + 4, ok)),
                                       ("cp_head_glove", "zg", head, (ok, ok + 4)),
                                       ("cp_head_glove", "z", head, (ok + 12, ok + 12))):
            rc = call(*ptrs)
            msg = lib.cp_last_error()
            assert rc == 10001, (entry, arg, dtype, rc, msg)
            assert entry.encode() in msg and (b" " + arg.encode() + b" must be 16-byte aligned") in msg, (entry, arg, msg)


def test_onehot_heads_refuse_ragged_views_and_misaligned_z_before_they_launch(lib):
    """cp_head and cp_head_gneg run the kernel that cp_head_glove runs: group g reads the z rows of batch entry g / V in 16-byte
    pieces.  An n_groups that is no multiple of V (the last batch entry's rows would lie past n_windows) and a z that is 4, 8 or 12
    bytes off are refused with CP_ERR_ARG and a message that names the entry, before any launch (every pointer is a dummy address
    that is never dereferenced; sizes and the workspace are valid, so the check under test is what refuses)"""
    from contrastiveprosthetics_amd import _lib
    ok, ws = 0x100000, 0x40000000
    pp = _lib.cp_params()
    pp.easy_w = pp.easy_b = ok
    for dtype in (0, 1, 2):                                       # CP_F32, CP_BF16, CP_FP8
        for groups, V in ((3, 2), (25, 3), (26, 25)):
            cfg = _lib.cp_config()
            cfg.n_windows, cfg.dtype = 41 * groups, dtype
            nb = lib.cp_workspace_bytes(cfg.n_windows, dtype, 0.0)

            def head(z, v, want_grad=0):
                return lib.cp_head(ctypes.byref(cfg), ctypes.byref(pp), z, ok, groups, v, want_grad, ws, nb, ok, ok, None,
                                   ctypes.byref(pp), None)

            def gneg(z, v, want_grad=0):
                return lib.cp_head_gneg(ctypes.byref(cfg), ctypes.byref(pp), z, ok, groups, v, want_grad, ws, nb, ok, ok, None,
                                        ctypes.byref(pp), ok, None)

            for want_grad in (0, 1):
                rc = head(ok, V, want_grad)
                assert rc == 10001 and b"cp_head args" in lib.cp_last_error(), (dtype, groups, V, rc, lib.cp_last_error())
                rc = gneg(ok, V, want_grad)                       # (the extension takes training batches, V == 1: no ragged view exists)
                assert rc == 10001 and b"cp_head_gneg" in lib.cp_last_error(), (dtype, groups, V, rc, lib.cp_last_error())
            for entry, call in (("cp_head", head), ("cp_head_gneg", gneg)):
                for off in (4, 8, 12):
                    rc = call(ok + off, 1)
                    msg = lib.cp_last_error()
                    assert rc == 10001, (entry, dtype, off, rc, msg)
                    assert entry.encode() + b": z must be 16-byte aligned" in msg, (entry, msg)


def test_head_grad_readback_refuses_null_out_and_short_workspaces_before_it_launches(lib):
    """cp_debug_head_grad / cp_debug_glove_head_grad validate as the calls whose rows they read: a NULL `out` is CP_ERR_ARG with the
    entry's name, a workspace one byte short CP_ERR_WORKSPACE (10002), a row count that is no multiple of 41 CP_ERR_ARG -- all
    before the conversion launch (dummy addresses, no GPU here)"""
    from contrastiveprosthetics_amd import _lib
    ok, ws, gws = 0x100000, 0x40000000, 0x200000
    for dtype in (0, 1, 2):
        rows = 41 * 5
        cfg = _lib.cp_config()
        cfg.n_windows, cfg.dtype = rows, dtype
        nb, gnb = lib.cp_workspace_bytes(rows, dtype, 0.0), lib.cp_glove_workspace_bytes(rows, dtype)
        rc = lib.cp_debug_head_grad(ctypes.byref(cfg), ws, nb, None, None)
        assert rc == 10001 and b"cp_debug_head_grad" in lib.cp_last_error(), (dtype, rc, lib.cp_last_error())
        rc = lib.cp_debug_glove_head_grad(ctypes.byref(cfg), gws, gnb, rows, None, None)
        assert rc == 10001 and b"cp_debug_glove_head_grad" in lib.cp_last_error(), (dtype, rc, lib.cp_last_error())
        rc = lib.cp_debug_head_grad(ctypes.byref(cfg), ws, nb - 1, ok, None)
        assert rc == 10002 and b"workspace too small" in lib.cp_last_error(), (dtype, rc, lib.cp_last_error())
        rc = lib.cp_debug_glove_head_grad(ctypes.byref(cfg), gws, gnb - 1, rows, ok, None)
        assert rc == 10002 and b"glove workspace too small" in lib.cp_last_error(), (dtype, rc, lib.cp_last_error())
        assert lib.cp_debug_head_grad(ctypes.byref(cfg), None, nb, ok, None) == 10001
        assert lib.cp_debug_glove_head_grad(ctypes.byref(cfg), gws, gnb, rows + 1, ok, None) == 10001
        assert lib.cp_debug_glove_head_grad(ctypes.byref(cfg), None, gnb, rows, ok, None) == 10001


def test_debug_fc_gemm_refuses_what_a_launcher_would_before_it_launches(lib):
    """cp_debug_fc_gemm checks its arguments on the host: what a launcher would refuse, or a kernel would read or write out of
    bounds, is CP_ERR_ARG with a message that names the entry, before any launch (every pointer is a dummy address that is never
    dereferenced; each case differs from a valid call in the one field under test, so that check is what refuses.  That the valid
    calls are accepted is shown on the GPU: tests/test_gpu_fc_gemm_exact.py).  cp_debug_gemm keeps refusing what it refused."""
    from contrastiveprosthetics_amd import _lib
    ok = 0x100000
    rows = ctypes.c_int32(-7)

    def call(**kw):
        d = _lib.cp_debug_fc_gemm_args()
        d.dtype, d.kind, d.M, d.K, d.F, d.tile_schedule = 1, 0, 1000, 512, 512, 0
        d.A = d.W = d.C = d.partials = ok
        d.stat_rows_out = ctypes.pointer(rows)
        for k, v in kw.items():
            setattr(d, k, v)
        if d.kind == 0 and "bias" not in kw:
            d.bias = ok
        rc = lib.cp_debug_fc_gemm(ctypes.byref(d), None)
        return rc, lib.cp_last_error()

    bn = dict(kind=1, R=ok, coef=ok, coef_mod=512)
    st = dict(kind=1, R=ok, dp_thresh=32768, dp_key=7, dp_inv_keep=2.0)
    cases = [("A", dict(A=None)), ("W", dict(W=None)), ("C", dict(C=None)), ("partials", dict(partials=None)),
             ("partials, kind 1", dict(kind=1, partials=None)), ("bias", dict(bias=None)),
             ("M = 0", dict(M=0)), ("M < 0", dict(M=-5)), ("K % 64", dict(K=544)), ("K = 0", dict(K=0)), ("F % 256", dict(F=640)),
             ("F = 0", dict(F=0)), ("F = 1024 forward", dict(F=1024)), ("F = 1024 plain dgrad", dict(kind=1, F=1024)),
             ("F = 1024 BN", dict(bn, F=1024)), ("F = 1024 ST", dict(st, F=1024)),
             ("kind 3", dict(kind=3)), ("kind -1", dict(kind=-1)), ("schedule 2", dict(tile_schedule=2)),
             ("schedule -1", dict(tile_schedule=-1)), ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
             ("coef_mod 0", dict(bn, coef_mod=0)), ("coef_mod -64", dict(bn, coef_mod=-64)),
             ("coef without R", dict(bn, R=None)), ("dropout without R", dict(st, R=None)), ("coef and dropout", dict(bn, **st)),
             ("coef in f32", dict(bn, dtype=0)), ("dropout in f32", dict(st, dtype=0)),
             ("R in the forward", dict(R=ok)), ("coef in the forward", dict(coef=ok, coef_mod=512)),
             ("dropout in the weight gradient", dict(st, kind=2)),
             ("dp_thresh 65536", dict(st, dp_thresh=65536)), ("dp_inv_keep 0", dict(st, dp_inv_keep=0.0)),
             ("K = 64 weight gradient", dict(kind=2, K=64)), ("K = 384 weight gradient", dict(kind=2, K=384)),
             ("K = 64 weight gradient, f32", dict(kind=2, K=64, dtype=0)),
             ("2^32 bytes", dict(M=2796203, K=768)), ("A + 8", dict(A=ok + 8)), ("W + 2", dict(W=ok + 2)), ("C + 4", dict(C=ok + 4)),
             ("R + 8", dict(bn, R=ok + 8))]
    for what, kw in cases:
        rc, msg = call(**kw)
        assert rc == 10001 and msg.startswith(b"cp_debug_fc_gemm"), (what, rc, msg)
        assert rows.value == -7, what
    for what, says in (("coef_mod 0", b"coef_mod"), ("F = 1024 BN", b"F > 768"), ("schedule 2", b"tile_schedule"), ("kind 3", b"kind")):
        assert says in call(**dict(cases)[what])[1], what
    assert lib.cp_debug_fc_gemm(None, None) == 10001
    for kw in (dict(A=None), dict(W=None), dict(C=None), dict(partials=None), dict(M=0), dict(K=544), dict(F=640), dict(kind=3)):
        a = dict(dtype=1, kind=0, M=1000, K=512, F=512, A=ok, W=ok, C=ok, bias=ok, R=None, partials=ok)
        a.update(kw)
        rc = lib.cp_debug_gemm(a["dtype"], a["kind"], a["M"], a["K"], a["F"], a["A"], a["W"], a["C"], a["bias"], a["R"], a["partials"], None)
        assert rc == 10001 and b"cp_debug_gemm args" in lib.cp_last_error(), (kw, rc, lib.cp_last_error())


def test_debug_conv_refuses_what_a_launcher_would_before_it_launches(lib):
    """cp_debug_conv checks its arguments on the host, before any launch: CP_ERR_ARG with a message that names the entry (every
    pointer is a dummy address that is never dereferenced; each case differs from a valid call of its kind in the one field under
    test.  That the valid calls are accepted is shown on the GPU: tests/test_gpu_conv_exact.py).  The ctypes struct follows the
    header field by field."""
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = hdr[hdr.index("typedef struct cp_debug_conv_args {"):hdr.index("} cp_debug_conv_args;")]
    assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in _lib.cp_debug_conv_args._fields_]
    assert ctypes.sizeof(_lib.cp_debug_conv_args) == 8 + 8 + 17 * 8 + 2 * 4 + 2 * 8
    ok = 0x100000
    rows, grows = ctypes.c_int32(-7), ctypes.c_int32(-9)
    pointers = ("x", "conv1_w", "conv1_b", "conv2_w", "conv2_b", "stats1", "gin", "coef", "wc", "out", "partials", "slabs", "fold", "dw", "db")

    def call(**kw):
        d = _lib.cp_debug_conv_args()
        d.dtype, d.kind, d.n_windows = 1, 0, 1000
        for name in pointers:
            setattr(d, name, ok)
        d.rows_out, d.gcol_rows_out = ctypes.pointer(rows), ctypes.pointer(grows)
        for k, v in kw.items():
            setattr(d, k, v)
        rc = lib.cp_debug_conv(ctypes.byref(d), None)
        return rc, lib.cp_last_error()

    e5 = dict(gin_exp=ok, gcols=ok, gcol_rows=3)
    cases = [("n_windows = 0", dict(n_windows=0)), ("n_windows < 0", dict(n_windows=-41)),
             ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)), ("kind 5", dict(kind=5)), ("kind -1", dict(kind=-1))]
    # every pointer a kind reads or writes
    needs = {0: ("x", "conv1_w", "conv1_b", "partials"),
             1: ("x", "conv1_w", "conv1_b", "conv2_w", "conv2_b", "stats1", "wc", "out", "partials"),
             2: ("x", "conv1_w", "conv1_b", "conv2_w", "gin", "wc", "out", "partials"),
             3: ("x", "conv1_w", "conv1_b", "conv2_w", "stats1", "gin", "partials", "slabs", "fold", "dw"),
             4: ("x", "conv1_w", "conv1_b", "conv2_w", "gin", "coef", "wc", "partials", "fold", "dw", "db")}
    for kind, names in needs.items():
        cases += [("kind %d without %s" % (kind, name), {"kind": kind, name: None}) for name in names]
    cases += [("kind 3 with gcols: slabs", dict(kind=3, gcols=ok, gcol_rows=3, slabs=None)),
              ("gcols without rows", dict(kind=3, gcols=ok, gcol_rows=0)), ("gcols with -1 rows", dict(kind=3, gcols=ok, gcol_rows=-1)),
              ("e5m2 in f32, kind 3", dict(e5, kind=3, dtype=0)), ("e5m2 in f32, kind 4", dict(kind=4, gin_exp=ok, dtype=0)),
              ("e5m2 without gcols", dict(kind=3, gin_exp=ok)),
              ("e5m2 in kind 0", dict(kind=0, gin_exp=ok)), ("e5m2 in kind 1", dict(kind=1, gin_exp=ok)), ("e5m2 in kind 2", dict(kind=2, gin_exp=ok)),
              ("2^32 bytes, bf16", dict(n_windows=2796203)), ("2^32 bytes, f32", dict(dtype=0, n_windows=1398102)),
              ("x + 8", dict(x=ok + 8)), ("gin + 8", dict(kind=2, gin=ok + 8)), ("out + 4", dict(kind=1, out=ok + 4)),
              ("wc + 2", dict(kind=4, wc=ok + 2)), ("gcols + 4", dict(kind=3, gcols=ok + 4, gcol_rows=3)),
              ("partials + 4", dict(partials=ok + 4)), ("slabs + 8", dict(kind=3, slabs=ok + 8)), ("fold + 4", dict(kind=4, fold=ok + 4))]
    for what, kw in cases:
        rc, msg = call(**kw)
        assert rc == 10001 and msg.startswith(b"cp_debug_conv"), (what, rc, msg)
        assert rows.value == -7 and grows.value == -9, what
    for what, says in (("kind 5", b"kind"), ("dtype 2", b"dtype"), ("e5m2 without gcols", b"gcols"), ("2^32 bytes, bf16", b"2^32"),
                       ("x + 8", b"aligned"), ("n_windows = 0", b"n_windows")):
        assert says in call(**dict(cases)[what])[1], what
    assert lib.cp_debug_conv(None, None) == 10001


def test_debug_proj_refuses_what_a_launcher_would_before_it_launches(lib):
    """cp_debug_proj checks its arguments on the host, before any launch: CP_ERR_ARG with a message that names the entry (every
    pointer is a dummy address that is never dereferenced; each case differs from a valid call of its kind in the one field under
    test -- kinds 2..4 carry a dropout, kind 1 none.  That the valid calls are accepted is shown on the GPU:
    tests/test_gpu_proj_exact.py).  The ctypes struct follows the header field by field."""
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = hdr[hdr.index("typedef struct cp_debug_proj_args {"):hdr.index("} cp_debug_proj_args;")]
    assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in _lib.cp_debug_proj_args._fields_]
    assert ctypes.sizeof(_lib.cp_debug_proj_args) == 8 + 8 + 14 * 8 + 4 * 4 + 8
    ok = 0x100000
    rows = ctypes.c_int32(-7)
    pointers = ("Wp", "act", "dz", "scale", "shift", "coef", "w32", "blast", "out", "slabs", "partials", "praw", "dzsum")
    drop = dict(dp_thresh=32768, dp_key=7, dp_inv_keep=2.0)

    def call(**kw):
        d = _lib.cp_debug_proj_args()
        d.dtype, d.kind, d.M = 1, kw.get("kind", 0), 1000
        for name in pointers:
            setattr(d, name, ok)
        d.rows_out = ctypes.pointer(rows)
        if d.kind >= 2:
            d.dp_thresh, d.dp_key, d.dp_inv_keep = 32768, 7, 2.0
        for k, v in kw.items():
            setattr(d, k, v)
        rc = lib.cp_debug_proj(ctypes.byref(d), None)
        return rc, lib.cp_last_error()

    cases = [("M = 0", dict(M=0)), ("M < 0", dict(M=-41)), ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
             ("kind 5", dict(kind=5)), ("kind -1", dict(kind=-1))]
    # every pointer a kind reads or writes
    needs = {0: ("Wp", "act", "scale", "shift", "w32", "blast", "out"),
             1: ("Wp", "act", "dz", "scale", "shift", "out", "slabs", "partials", "praw", "dzsum"),
             2: ("Wp", "act", "dz", "scale", "shift", "out", "slabs"),
             3: ("Wp", "act", "dz", "scale", "shift", "out", "slabs", "partials"),
             4: ("Wp", "act", "dz", "coef", "w32", "out", "partials")}
    for kind, names in needs.items():
        cases += [("kind %d without %s" % (kind, name), {"kind": kind, name: None}) for name in names]
    cases += [("kind 0 with dropout, without scale", dict(drop, scale=None)),
              ("kind 3 in f32", dict(kind=3, dtype=0)), ("kind 4 in f32", dict(kind=4, dtype=0)),
              ("e4m3 in f32, kind 0", dict(kind=0, dtype=0, r_exp=ok)), ("e4m3 in f32, kind 1", dict(kind=1, dtype=0, r_exp=ok)),
              ("e4m3 in kind 2", dict(kind=2, r_exp=ok)), ("e4m3 in kind 4", dict(kind=4, r_exp=ok)),
              ("dropout in kind 1", dict(drop, kind=1)), ("a key in kind 1", dict(kind=1, dp_key=7)),
              ("1 / (1 - p) in kind 1", dict(kind=1, dp_inv_keep=2.0)), ("a key without a threshold, kind 0", dict(dp_key=7)),
              ("1 / (1 - p) without a threshold, kind 0", dict(dp_inv_keep=2.0)),
              ("kind 2 without dropout", dict(kind=2, dp_thresh=0)), ("kind 3 without dropout", dict(kind=3, dp_thresh=0)),
              ("kind 4 without dropout", dict(kind=4, dp_thresh=0)),
              ("dp_thresh 65536, kind 0", dict(drop, dp_thresh=65536)), ("dp_inv_keep 0, kind 0", dict(drop, dp_inv_keep=0.0)),
              ("dp_inv_keep < 0, kind 0", dict(drop, dp_inv_keep=-2.0)),
              ("2^32 bytes, bf16", dict(M=4193280)), ("2^32 bytes, f32", dict(dtype=0, M=2096640)),
              ("2^32 bytes, kind 4", dict(kind=4, M=4193280)), ("M = 2^54: the byte count wraps to 0", dict(M=1 << 54)),
              ("M = 2^63 - 1", dict(M=(1 << 63) - 1))]
    for kind in range(2, 5):
        cases += [("dp_thresh 65536, kind %d" % kind, dict(kind=kind, dp_thresh=65536)),
                  ("dp_inv_keep 0, kind %d" % kind, dict(kind=kind, dp_inv_keep=0.0))]
    cases += [("%s + %d" % (name, off), {"kind": kind, name: ok + off})
              for name, kind, off in (("Wp", 0, 4), ("act", 0, 8), ("dz", 1, 8), ("scale", 0, 4), ("shift", 2, 8), ("coef", 4, 4), ("w32", 4, 2),
                                      ("blast", 0, 4), ("out", 0, 8), ("slabs", 3, 4), ("partials", 4, 8), ("praw", 1, 4), ("dzsum", 1, 4))]
    for what, kw in cases:
        rc, msg = call(**kw)
        assert rc == 10001 and msg.startswith(b"cp_debug_proj"), (what, rc, msg)
        assert rows.value == -7, what
    for what, says in (("kind 5", b"kind"), ("dtype 2", b"dtype"), ("e4m3 in kind 2", b"r_exp"), ("2^32 bytes, bf16", b"2^32"),
                       ("Wp + 4", b"aligned"), ("M = 0", b"M must"), ("dropout in kind 1", b"no dropout"),
                       ("kind 3 without dropout", b"behind a dropout"), ("kind 4 in f32", b"CP_BF16"), ("dp_thresh 65536, kind 3", b"dp_thresh")):
        assert says in call(**dict(cases)[what])[1], what
    assert lib.cp_debug_proj(None, None) == 10001


def test_debug_bn_refuses_what_a_launcher_would_before_it_launches(lib):
    """cp_debug_bn checks its arguments on the host, before any launch: CP_ERR_ARG with a message that names the entry (every device
    pointer is a dummy address that is never dereferenced; params and bn are real host structs of such addresses; each case differs
    from a valid call of its kind in the one field under test.  That the valid calls are accepted is shown on the GPU:
    tests/test_gpu_bn_exact.py).  The ctypes struct follows the header field by field."""
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = hdr[hdr.index("typedef struct cp_debug_bn_args {"):hdr.index("} cp_debug_bn_args;")]
    assert re.findall(r"\b(\w+)(?:\[[^\]]*\])?\s*;", body) == [f[0] for f in _lib.cp_debug_bn_args._fields_]
    assert ctypes.sizeof(_lib.cp_debug_bn_args) == 8 * 4 + 8 + 8 + 6 * 4 + 22 * 8 + (9 + 8 + 8) * 8 + 8
    ok = 0x100000
    rows = ctypes.c_int32(-7)
    pointers = ("rows", "gamma", "beta", "running_mean", "running_var", "scratch", "stats", "coef", "dgamma", "dbeta", "r", "g",
                "partials", "db", "W", "b", "s", "t")

    def call(**kw):
        kw = dict(kw)
        d = _lib.cp_debug_bn_args()
        d.dtype, d.kind, d.M, d.C, d.nfold, d.K, d.count = 1, kw.get("kind", 0), 1000, 512, 1, 512, 4096.0
        d.momentum, d.eps, d.update_running = 0.5, 1e-5, 1
        d.dp_thresh, d.dp_key, d.dp_inv_keep = 32768, 7, 2.0
        p, bn = _lib.cp_params(), _lib.cp_bn_buffers()
        for i in range(7):
            p.fc_w[i], p.fc_b[i] = ok, ok
        for l in range(9):
            p.bn_g[l], p.bn_b[l], bn.running_mean[l], bn.running_var[l], d.stats9[l] = ok, ok, ok, ok, ok
        p.last_w = ok
        for i in range(8):
            d.wimg[i], d.bimg[i] = ok, ok
        d.params, d.bn = ctypes.addressof(p), ctypes.addressof(bn)
        for name in pointers:
            setattr(d, name, ok)
        d.rows_out = ctypes.pointer(rows)
        for path in kw.pop("clear", ()):                 # a member of params, bn or an array: ("fc_w", 3) | ("stats9", 2) | ("last_w",)
            tgt = p if hasattr(p, path[0]) else (bn if hasattr(bn, path[0]) else d)
            if len(path) == 2:
                getattr(tgt, path[0])[path[1]] = kw.get("to", None)
            else:
                setattr(tgt, path[0], kw.get("to", None))
        kw.pop("to", None)
        for k, v in kw.items():
            setattr(d, k, v)
        rc = lib.cp_debug_bn(ctypes.byref(d), None)
        return rc, lib.cp_last_error()

    cases = [("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)), ("kind 6", dict(kind=6)), ("kind -1", dict(kind=-1)),
             ("mode 1 outside kind 5", dict(kind=0, mode=1)), ("mode 4", dict(kind=5, mode=4)), ("mode -1", dict(kind=5, mode=-1))]
    for kind in (0, 2, 3, 4):
        cases += [("M = 0, kind %d" % kind, dict(kind=kind, M=0)), ("M < 0, kind %d" % kind, dict(kind=kind, M=-41))]
    for kind in (0, 2, 4):
        cases += [("C = 128, kind %d" % kind, dict(kind=kind, C=128)), ("C = 0, kind %d" % kind, dict(kind=kind, C=0))]
    cases += [("nfold 12 at C = 512", dict(kind=2, nfold=12)), ("nfold 2", dict(kind=2, C=64, nfold=2)), ("nfold 0", dict(kind=2, nfold=0)),
              ("K = 640", dict(kind=5, K=640)), ("K = 512 in mode 1", dict(kind=5, mode=1, K=512)),
              ("count 0", dict(count=0.0)), ("count nan, kind 2", dict(kind=2, count=float("nan"))),
              ("2^31 partial rows", dict(M=1 << 31)), ("2^31 partial rows, kind 2", dict(kind=2, M=1 << 31)),
              ("update_running without buffers", dict(running_mean=None, running_var=None)),
              ("running_mean alone", dict(running_var=None, update_running=0)), ("unscale_exp + 2", dict(unscale_exp=ok + 2)),
              ("s without t", dict(kind=5, t=None)), ("t without s", dict(kind=5, mode=1, K=768, s=None)),
              ("params NULL, kind 1", dict(kind=1, params=None)), ("bn NULL", dict(kind=1, bn=None)),
              ("params NULL, mode 2", dict(kind=5, mode=2, params=None)), ("params NULL, mode 3", dict(kind=5, mode=3, params=None)),
              ("dp_thresh 65536", dict(kind=3, dp_thresh=65536)), ("dp_inv_keep 0", dict(kind=3, dp_inv_keep=0.0)),
              ("dp_inv_keep < 0", dict(kind=3, dp_inv_keep=-2.0)),
              ("2^32 bytes, bf16, kind 3", dict(kind=3, M=4193280)), ("2^32 bytes, f32, kind 3", dict(kind=3, dtype=0, M=2096640)),
              ("2^32 bytes, bf16, kind 4", dict(kind=4, M=4193280)), ("2^32 bytes, f32, C = 64", dict(kind=4, dtype=0, C=64, M=16773120)),
              ("M = 2^54: the byte count wraps to 0", dict(kind=4, M=1 << 54)), ("M = 2^63 - 1", dict(kind=3, M=(1 << 63) - 1))]
    # every pointer a kind reads or writes
    needs = {0: ("rows", "gamma", "beta", "scratch", "stats"), 2: ("rows", "scratch", "stats", "coef", "dgamma", "dbeta"),
             3: ("r", "stats", "g"), 4: ("r", "g", "coef", "partials", "scratch", "db")}
    for kind, names in needs.items():
        cases += [("kind %d without %s" % (kind, name), {"kind": kind, name: None}) for name in names]
    cases += [("mode %d without %s" % (mode, name), {"kind": 5, "mode": mode, "K": 768, name: None}) for mode in (0, 1) for name in ("W", "b")]
    cases += [("mode 0 without its image", dict(kind=5, clear=[("wimg", 0)])), ("mode 1 without its bias", dict(kind=5, mode=1, K=768, clear=[("bimg", 0)]))]
    for member in ("fc_w", "fc_b", "wimg", "bimg"):
        cases += [("kind 1 without %s[%d]" % (member, i), dict(kind=1, clear=[(member, i)])) for i in (0, 6)]
        cases += [("mode 2 without %s[%d]" % (member, i), dict(kind=5, mode=2, clear=[(member, i)])) for i in (4, 6)]
    for member in ("fc_w", "wimg"):
        cases += [("mode 3 without %s[%d]" % (member, i), dict(kind=5, mode=3, clear=[(member, i)])) for i in (0, 6)]
    for kind, mode in ((1, 0), (5, 2), (5, 3)):
        cases += [("kind %d mode %d without last_w" % (kind, mode), dict(kind=kind, mode=mode, clear=[("last_w",)])),
                  ("kind %d mode %d without wimg[7]" % (kind, mode), dict(kind=kind, mode=mode, clear=[("wimg", 7)]))]
    cases += [("kind 1 without bimg[7]", dict(kind=1, clear=[("bimg", 7)])), ("mode 2 without bimg[7]", dict(kind=5, mode=2, clear=[("bimg", 7)]))]
    for member in ("bn_g", "bn_b", "running_mean", "running_var", "stats9"):
        cases += [("kind 1 without %s[%d]" % (member, l), dict(kind=1, clear=[(member, l)])) for l in (0, 8)]
    cases += [("%s + %d, kind %d" % (name, off, kind), {"kind": kind, name: ok + off})
              for name, kind, off in (("rows", 0, 4), ("gamma", 0, 4), ("beta", 0, 8), ("running_mean", 0, 4), ("running_var", 0, 8), ("scratch", 2, 4),
                                      ("stats", 3, 8), ("local", 2, 4), ("coef", 4, 4), ("dgamma", 2, 4), ("dbeta", 2, 8), ("r", 3, 2), ("g", 4, 8),
                                      ("partials", 4, 4), ("db", 4, 4), ("W", 5, 4), ("b", 5, 8), ("s", 5, 4), ("t", 5, 4))]
    cases += [("fc_w[2] + 4, kind 1", dict(kind=1, clear=[("fc_w", 2)], to=ok + 4)), ("wimg[7] + 2, mode 3", dict(kind=5, mode=3, clear=[("wimg", 7)], to=ok + 2)),
              ("stats9[8] + 8", dict(kind=1, clear=[("stats9", 8)], to=ok + 8)), ("running_var[1] + 4", dict(kind=1, clear=[("running_var", 1)], to=ok + 4))]
    for what, kw in cases:
        rc, msg = call(**kw)
        assert rc == 10001 and msg.startswith(b"cp_debug_bn"), (what, rc, msg)
        assert rows.value == -7, what
    for what, says in (("kind 6", b"kind"), ("dtype 2", b"dtype"), ("mode 4", b"mode"), ("C = 128, kind 4", b"C must"), ("nfold 2", b"nfold"),
                       ("K = 640", b"K must"), ("2^32 bytes, bf16, kind 3", b"2^32"), ("rows + 4, kind 0", b"aligned"), ("M = 0, kind 3", b"M must"),
                       ("dp_thresh 65536", b"dp_thresh"), ("s without t", b"together"), ("count 0", b"count"), ("bn NULL", b"bn must")):
        assert says in call(**dict(cases)[what])[1], what
    assert lib.cp_debug_bn(None, None) == 10001


def test_debug_fp8_refuses_what_a_launcher_would_before_it_launches(lib):
    """cp_debug_fp8 checks its arguments on the host, before any launch: CP_ERR_ARG with a message that names the entry (every
    pointer is a dummy address that is never dereferenced; each case differs from a valid call of its kind in the one field under
    test.  That the valid calls are accepted is shown on the GPU: tests/test_gpu_fp8_exact.py).  The ctypes struct follows the header
    field by field."""
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = hdr[hdr.index("typedef struct cp_debug_fp8_args {"):hdr.index("} cp_debug_fp8_args;")]
    assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in _lib.cp_debug_fp8_args._fields_]
    assert ctypes.sizeof(_lib.cp_debug_fp8_args) == 2 * 4 + 8 + 8 * 4 + 16 * 8 + 4 * 4 + 8
    ok = 0x100000
    rows = ctypes.c_int32(-7)
    pointers = ("state", "A", "W", "wsc", "bias", "R", "coef", "bn_stats", "scale", "shift", "C", "partials", "A2", "R2", "partials2", "C2")

    def call(**kw):
        d = _lib.cp_debug_fp8_args()
        d.kind, d.M, d.K, d.F, d.coef_mod = kw.get("kind", 0), 1000, 512, 512, 512
        d.t_in, d.t_r, d.t_out, d.t_in2, d.t_r2 = 1, 2, 3, 4, 5
        for name in pointers:
            setattr(d, name, ok)
        d.rows_out = ctypes.pointer(rows)
        d.dp_thresh, d.dp_key, d.dp_inv_keep = 32768, 7, 2.0
        for k, v in kw.items():
            setattr(d, k, v)
        rc = lib.cp_debug_fp8(ctypes.byref(d), None)
        return rc, lib.cp_last_error()

    cases = [("kind 9", dict(kind=9)), ("kind -1", dict(kind=-1)), ("mode 1 in kind 0", dict(mode=1)), ("mode 2 in kind 3", dict(kind=3, mode=2)),
             ("mode 4 in kind 7", dict(kind=7, mode=4)), ("mode -1 in kind 7", dict(kind=7, mode=-1))]
    for kind in range(9):
        cases += [("kind %d, M = 0" % kind, dict(kind=kind, M=0)), ("kind %d, M < 0" % kind, dict(kind=kind, M=-41)),
                  ("kind %d without state" % kind, dict(kind=kind, state=None)), ("kind %d, state + 4" % kind, dict(kind=kind, state=ok + 4)),
                  ("kind %d, dp_thresh 65536" % kind, dict(kind=kind, dp_thresh=65536))]
    # every pointer a kind reads or writes (kind 0 without partials is the evaluation form; kind 7's bias, scale and shift are optional)
    needs = {0: ("A", "W", "wsc", "bias", "C"), 1: ("A", "W", "wsc", "R", "coef", "C", "partials"),
             2: ("A", "W", "wsc", "R", "bn_stats", "C", "partials"), 3: ("A", "R", "C", "partials"), 4: ("A", "bn_stats", "C"),
             5: ("R", "coef", "C", "partials"), 6: ("A", "W", "R", "coef", "C", "partials"), 7: ("A", "wsc", "C", "partials")}
    for kind, names in needs.items():
        cases += [("kind %d without %s" % (kind, name), {"kind": kind, name: None}) for name in names]
        cases += [("kind %d, %s + 8" % (kind, name), {"kind": kind, name: ok + 8}) for name in names]
    cases += [("paired without %s" % name, {"kind": 3, "mode": 1, name: None}) for name in ("A2", "R2", "partials2", "C2")]
    cases += [("kind 7, scale without shift", dict(kind=7, shift=None)), ("kind 7, shift without scale", dict(kind=7, mode=1, scale=None))]
    # shapes
    cases += [("kind 0, K = 256", dict(K=256)), ("kind 0, K = 1024", dict(K=1024)), ("kind 0, F = 768", dict(F=768)), ("kind 0, F = 256", dict(F=256)),
              ("kind 1, F = 1024", dict(kind=1, F=1024)), ("kind 1, F = 256", dict(kind=1, F=256)), ("kind 1, F = 0", dict(kind=1, F=0)),
              ("kind 1, coef_mod 0", dict(kind=1, coef_mod=0)), ("kind 1, coef_mod < 0", dict(kind=1, coef_mod=-64)),
              ("kind 3, F = 640", dict(kind=3, F=640)), ("paired, F = 768", dict(kind=3, mode=1, F=768)),
              ("kind 7, K = 640", dict(kind=7, K=640)), ("kind 7 transposed, K = 0", dict(kind=7, mode=2, K=0))]
    cases += [("kind %d, F = 768" % kind, dict(kind=kind, F=768)) for kind in (2, 4, 5, 6)]
    # ids
    reads = {0: ("t_out",), 1: ("t_r", "t_out"), 2: ("t_r", "t_out"), 3: ("t_in", "t_r"), 4: ("t_in", "t_out"), 5: ("t_in", "t_r", "t_out"),
             6: ("t_r", "t_out"), 7: ("t_in", "t_out")}
    for kind, names in reads.items():
        cases += [("kind %d, %s = 64" % (kind, name), {"kind": kind, name: 64}) for name in names]
        cases += [("kind %d, %s = -1" % (kind, name), {"kind": kind, name: -1}) for name in names if (kind, name) != (7, "t_out")]
    cases += [("kind 7, t_out = -2", dict(kind=7, t_out=-2)), ("kind 7 transposed, t_in = 64", dict(kind=7, mode=2, t_in=64)),
              ("paired, t_in2 = 64", dict(kind=3, mode=1, t_in2=64)), ("paired, t_r2 = -1", dict(kind=3, mode=1, t_r2=-1))]
    # dropout
    cases += [("kind %d, dp_inv_keep 0" % kind, dict(kind=kind, dp_inv_keep=0.0)) for kind in (2, 4, 6)]
    cases += [("kind 4, dp_inv_keep < 0", dict(kind=4, dp_inv_keep=-2.0))]
    # 32-bit offsets: 0xFFF00000 / 512 = 8386560, / 768 = 5591040
    cases += [("kind %d, 2^32 bytes" % kind, dict(kind=kind, M=8386560)) for kind in range(7)]
    cases += [("kind 0, K = 768, 2^32 bytes", dict(K=768, M=5591040)), ("kind 1, F = 768, 2^32 bytes", dict(kind=1, F=768, M=5591040)),
              ("M = 2^54: the byte count wraps to 0", dict(M=1 << 54)), ("M = 2^63 - 1", dict(kind=2, M=(1 << 63) - 1))]
    for what, kw in cases:
        rc, msg = call(**kw)
        assert rc == 10001 and msg.startswith(b"cp_debug_fp8"), (what, rc, msg)
        assert rows.value == -7, what
    for what, says in (("kind 9", b"kind"), ("mode 1 in kind 0", b"mode"), ("kind 3, M = 0", b"M must"), ("kind 5 without state", b"state"),
                       ("kind 1 without coef", b"coef"), ("kind 2 without bn_stats", b"bn_stats"), ("paired without R2", b"R2"),
                       ("kind 0, K = 256", b"K = 512 | 768"), ("kind 4, F = 768", b"F = 512"), ("kind 1, coef_mod 0", b"coef_mod"),
                       ("kind 5, t_in = 64", b"t_in"), ("kind 6, t_r = -1", b"t_r"), ("kind 0, t_out = 64", b"t_out"), ("paired, t_in2 = 64", b"t_in2"),
                       ("kind 4, dp_thresh 65536", b"dp_thresh"), ("kind 2, dp_inv_keep 0", b"dp_inv_keep"), ("kind 6, 2^32 bytes", b"2^32"),
                       ("kind 3, R + 8", b"aligned"), ("kind 7, scale without shift", b"scale and shift")):
        assert says in call(**dict(cases)[what])[1], (what, call(**dict(cases)[what])[1])
    assert lib.cp_debug_fp8(None, None) == 10001


def test_backward_refuses_a_short_gradient_tap_before_it_launches(lib):
    """cp_config.grad_tap: cp_encoder_backward checks the whole buffer once, before its first launch -- 9 slots of n_windows x 768
    elements on the large-batch paths (CP_FP8: bf16 elements), 11 on the small-batch path (slot 9: fc1's data gradient before conv2's
    weight-gradient launch overwrites it).  One byte short returns CP_ERR_ARG and leaves the forward record untouched (every pointer
    is a dummy address that is never dereferenced: there is no GPU here, so a launch or a copy would fail with another code).  That a buffer
    of exactly the stated size is accepted is shown on the GPU: tests/test_gpu_small_recompute.py and tests/test_gpu_fullsize.py allocate
    exactly 11 and 9 slots."""
    from contrastiveprosthetics_amd import _lib
    ok, ws = 0x100000, 0x40000000
    #            groups, dtype, record path (PATH_LARGE 0, PATH_SMALL 1, PATH_FP8 2), slots, element bytes
    for groups, dtype, path, slots, es in ((8, 1, 1, 11, 2), (64, 0, 1, 11, 4), (65, 1, 0, 9, 2), (65, 0, 0, 9, 4), (8, 2, 2, 9, 2)):
        n = 41 * groups
        cfg = _lib.cp_config()
        cfg.n_windows, cfg.dtype, cfg.training, cfg.bn_momentum, cfg.bn_eps = n, dtype, 1, 0.1, 1e-5
        rec = _lib.cp_forward_record(n, path, 0, 0, 0, None)
        cfg.record = ctypes.pointer(rec)
        nb = lib.cp_workspace_bytes(n, dtype, 0.0)
        need = slots * n * 768 * es
        cfg.grad_tap = ok
        pp, gg = _lib.cp_params(), _lib.cp_params()
        for short in (need - 1, (slots - 1) * n * 768 * es, 0):
            cfg.grad_tap_bytes = short
            rc = lib.cp_encoder_backward_ev(ctypes.byref(cfg), ctypes.byref(pp), ok, ws, nb, ctypes.byref(gg), None, None)
            assert rc == 10001 and b"gradient tap buffer too small" in lib.cp_last_error(), (groups, dtype, short, rc, lib.cp_last_error())
            assert rec.backwards == 0


def test_optimiser_entries_refuse_bad_tables_before_they_launch(lib):
    """cp_l2_norms, cp_l2_adam_step and cp_l2_adam_step_graph take any tensor table of 1..64 entries; what the kernels cannot
    index is refused with CP_ERR_ARG and a message that names the entry, before any launch: no entry or 65, a negative numel
    (a negative chunk count: the grid would no longer match the table), a negative offset (an index in front of the buffers), a
    table without an element (an empty grid), and a step index of 0 (every pointer is a dummy address that is never
    dereferenced: there is no GPU here, so a launch would fail with another code)"""
    from contrastiveprosthetics_amd import _lib
    ok = 0x100000
    h = _lib.cp_adam_hyper(1e-3, 3e-2, 1e-3, 2e-2, 0.9, 0.999, 1e-8, 1.0)

    def arrays(off, numel):
        n = len(off)
        return ((ctypes.c_int64 * n)(*off), (ctypes.c_int64 * n)(*numel), (ctypes.c_int32 * n)(*([0, 1] * n)[:n]),
                (ctypes.c_int32 * n)(*([1, 0] * n)[:n]))

    def norms(tab, n, step=1):
        return lib.cp_l2_norms(ok, *tab, n, ctypes.byref(h), ok, ok, None)

    def plain(tab, n, step=1):
        return lib.cp_l2_adam_step(ok, ok, ok, ok, *tab, n, ctypes.byref(h), step, ok, ok, None)

    def graph(tab, n, step=1):
        return lib.cp_l2_adam_step_graph(ok, ok, ok, ok, *tab, n, ctypes.byref(h), ok, ok, ok, None)

    good = arrays([0, 64, 4160], [5, 4096, 1])
    many = arrays([64 * i for i in range(65)], [7] * 65)
    for entry, call in (("cp_l2_norms", norms), ("cp_l2_adam_step", plain), ("cp_l2_adam_step_graph", graph)):
        for what, tab, n, says in (("n = 0", good, 0, b"n = 0"),
                                   ("n = -1", good, -1, b"n = -1"),
                                   ("n = 65", many, 65, b"n = 65"),
                                   ("numel[1] = -1", arrays([0, 64, 4160], [5, -1, 1]), 3, b"entry 1 has a negative numel"),
                                   ("numel[2] = -4096", arrays([0, 64, 4160], [5, 4096, -4096]), 3, b"entry 2 has a negative numel"),
                                   ("offset[0] = -1", arrays([-1, 64, 4160], [5, 4096, 1]), 3, b"entry 0 has a negative offset"),
                                   ("offset[2] = -4", arrays([0, 64, -4], [5, 4096, 1]), 3, b"entry 2 has a negative offset"),
                                   ("no element", arrays([0, 64], [0, 0]), 2, b"without an element")):
            rc = call(tab, n)
            msg = lib.cp_last_error()
            assert rc == 10001, (entry, what, rc, msg)
            assert msg.startswith(entry.encode() + b":") and says in msg, (entry, what, msg)
        rc = lib.cp_l2_adam_step(ok, ok, ok, ok, None, good[1], good[2], good[3], 3, ctypes.byref(h), 1, ok, ok, None)
        assert rc == 10001 and b"cp_l2_adam_step: tensor table" in lib.cp_last_error()
    for step in (0, -1):
        rc = plain(good, 3, step=step)
        assert rc == 10001 and b"cp_l2_adam_step args" in lib.cp_last_error(), (step, rc, lib.cp_last_error())
    # (the graph form takes its step from the device state, the norms take none: a missing state is what they refuse)
    rc = lib.cp_l2_adam_step_graph(ok, ok, ok, ok, *good, 3, ctypes.byref(h), None, ok, ok, None)
    assert rc == 10001 and b"cp_l2_adam_step_graph args" in lib.cp_last_error()


def test_missing_library_is_an_error(monkeypatch):
    from contrastiveprosthetics_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libcpnative.so")
    with pytest.raises(_lib.CpNativeError):
        _lib.load()


def test_engine_refuses_cpu():
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.engine import Engine
    with pytest.raises(_lib.CpNativeError):
        Engine(adabn=True, dtype="f32", device="cpu")


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "contrastiveprosthetics_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("no oracle", ""), f"{f} mentions the oracle"


def test_constants_match_oracle_and_golden(golden_dir):
    from contrastiveprosthetics_amd import constants as c
    o = oc.split_constants()
    assert np.array_equal(c.d2_idxs, o["d2_idxs"]) and np.array_equal(c.d3_idxs, o["d3_idxs"])
    assert np.array_equal(c.TASKS, o["tasks"])
    g = np.load(os.path.join(golden_dir, "db23_sampler.npz"))
    assert np.array_equal(np.concatenate((c.TASKS, [0])), g["tasks_mask"])        # reference values
    assert np.array_equal(c.d3_idxs + 40, g["people_mask"])
    assert (c.MAX_TASKS, c.EMG_DIM, c.GLOVE_DIM, c.PREDICTION_WINDOW_SIZE, c.AMT_PREDICTION_WINDOWS) == (41, 12, 20, 25, 4)


@pytest.mark.parametrize("adabn", [False, True])
def test_param_table_matches_reference_state_dict(adabn):
    from contrastiveprosthetics_amd.engine import l2_member, param_specs
    specs = param_specs(adabn)
    ref = oc.init_state_dict(0, 16, adabn)
    ref_params = [k for k, v in ref.items() if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var"))
                  and k != "logit_scale"]
    assert list(specs) == ref_params
    for k in specs:
        assert tuple(ref[k].shape) == tuple(specs[k])
    m = oc.OracleModel(ref, dict(reg_emg=1, reg_glove=1), adabn=adabn)
    emg, glove = m.l2_keys()
    assert sorted(k for k in specs if l2_member(k)) == sorted(emg + glove)
    assert sum(int(np.prod(s)) for s in specs.values()) == 2027616


def test_cli_surface_matches_reference():
    from contrastiveprosthetics_amd.train import build_parser
    a = build_parser().parse_args([])
    assert (a.crossval_size, a.crossval_epochs, a.batch_size, a.final_epochs) == (10, 1, 32, 10)
    assert (a.glove, a.db2, a.load_model, a.crossval_load, a.prediction, a.test) == (False,) * 6
    assert (a.no_adabn, a.no_checkpoint, a.no_verbose) == (True, True, True)          # store_false polarity
    b = build_parser().parse_args(["--no_adabn", "--no_checkpoint", "--no_verbose", "--test", "--batch_size=8"])
    assert (b.no_adabn, b.no_checkpoint, b.no_verbose, b.test, b.batch_size) == (False, False, False, True, 8)


def test_shard_range_partitions():
    from contrastiveprosthetics_amd.dist import shard_range
    for n in (0, 1, 7, 8, 4096, 1801):
        for w in (1, 2, 3, 8):
            spans = [shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            sizes = [e - s for s, e in spans]
            assert max(sizes) - min(sizes) <= 1


@pytest.mark.parametrize("final_epochs", [8, 12])
def test_lr_closed_forms_equal_the_reference_schedulers(final_epochs):
    """train.lr_scales against torch.optim.lr_scheduler objects built exactly as code/train.py:75-80 builds them and
    stepped once per epoch as at :112-113: CosineAnnealingLR(T_max=final_epochs, eta_min=0) on both optimisers when
    annealing, else two StepLR(step_size=5, gamma=.2) that BOTH wrap optimizer_glove (the reference's quirk: the emg
    rate never moves, the glove rate falls by .2**2 every 5 epochs)."""
    import torch.optim as optim
    from contrastiveprosthetics_amd.train import lr_scales
    lr_e, lr_g = 9.761e-4, 2.653e-3
    for annealing in (True, False):
        pe, pg = torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))
        oe = optim.Adam([pe], lr=lr_e, weight_decay=0)
        og = optim.Adam([pg], lr=lr_g, weight_decay=0)
        if annealing:
            se = optim.lr_scheduler.CosineAnnealingLR(oe, T_max=final_epochs, eta_min=0)
            sg = optim.lr_scheduler.CosineAnnealingLR(og, T_max=final_epochs, eta_min=0)
        else:
            se = optim.lr_scheduler.StepLR(og, step_size=5, gamma=.2)
            sg = optim.lr_scheduler.StepLR(og, step_size=5, gamma=.2)
        for epoch in range(12):
            s = lr_scales(epoch, annealing, final_epochs)
            assert oe.param_groups[0]["lr"] == pytest.approx(lr_e * s[0], rel=1e-6, abs=1e-12), (annealing, epoch)
            assert og.param_groups[0]["lr"] == pytest.approx(lr_g * s[1], rel=1e-6, abs=1e-12), (annealing, epoch)
            oe.step(); og.step()
            se.step(); sg.step()


def test_register_stationary_gemm_kernel_has_no_spills():
    """The weight-stationary GEMM kernels (csrc/gemm_ws.cuh: gemm_ws16_kernel, gemm_ws16n_kernel, gemm_wsd16_kernel<0|1>; csrc/fp8.cuh:
    gemm_ws8_kernel<512|768>, gemm_wsd8_kernel<0|1>) keep 128-256 weight registers per wave and run at the edge of the 512-register file.  A spill costs them their
    speed (scratch traffic inside the k loop), and in round 2 every build that spilled also returned wrong values -- that turned out to be
    the store-data hazard that csrc/gemm_ws.cuh::store_b128_settled now closes, not the spills themselves; the guard stays for the speed:
    hipcc's resource remarks are checked at build time."""
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "gemm_wsd?(16n?|8)?_kernel"], capture_output=True, text=True,
                         check=True).stdout
    lines = [l for l in out.splitlines() if "gemm_ws" in l]
    assert len(lines) >= 8, out          # (ws16, ws16n, wsd16<0|1>, ws8<512|768>, wsd8<0|1>)
    for l in lines:
        assert re.search(r"spill\s+0\s+scratch\s+0\b", l), l


def test_library_assembly_has_no_buffer_store_data_hazard():
    """gfx950 store-data hazard (csrc/gemm_ws.cuh, store_b128_settled; DESIGN.md section 4, "The lanes 12-15 fault"): hipcc places a
    VALU write of a buffer_store_dwordx4's data registers directly behind the store when the store's soffset is an SGPR, and the
    store then sends the new values for some lanes.  tools/store_hazard_scan.py reads the device assembly of the whole library: no
    96/128-bit buffer store may have such a write within the next two instructions."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "store_hazard_scan.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().startswith("0 unprotected"), out.stdout[-500:]


def test_pinned_mfmas_keep_their_wait_states():
    """The 8-bit weight-stationary kernels (csrc/fp8.cuh: gemm_ws8_kernel, gemm_wsd8_kernel) issue their MFMAs as volatile asm statements so
    that the previous tile's epilogue can be paced between them; hipcc's hazard tables do not see inside such a statement.
    tools/pinned_mfma_audit.py reads the device assembly: no vector write of an operand within two states in front of a pinned MFMA, no
    vector write of a C operand that is not the destination within seven states behind it, no scratch in those kernels."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pinned_mfma_audit.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    first = out.stdout.strip().split("\n")[0]
    assert first.endswith("0 finding(s)") and int(first.split()[0]) >= 6, out.stdout[-500:]


def test_library_never_reads_the_environment():
    """no getenv anywhere in the library (sources and the .so's imports): a call's settings travel in its cp_config"""
    import glob
    hits = []
    for f in glob.glob(os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc", "*")):
        for i, line in enumerate(open(f, errors="replace")):
            if "getenv(" in line and not line.lstrip().startswith("//"):
                hits.append((os.path.basename(f), i + 1, line.strip()))
    assert hits == [], hits
    src = open(os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc", "api.hip")).read()
    # and nothing process-wide is left for the training path to consult
    assert not re.search(r"^static [^(]*\bg_(opt|sync_fn|sync_user|sync_world|grad_tap|tile_schedule|notes)\b", src, flags=re.M)
    # what a forward pass leaves for the backward is the caller's cp_forward_record, not a table keyed by workspace address
    assert "g_notes" not in src and "FwdNote" not in src and "std::mutex" not in src
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout


def test_library_sources_have_no_preprocessor_conditionals():
    """every line under csrc/ is compiled into libcpnative.so: no build-time switches, no code only another build sees"""
    import glob
    hits = []
    for f in glob.glob(os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc", "*")):
        if f.endswith((".hip", ".cuh")):
            for i, line in enumerate(open(f, errors="replace")):
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", line):
                    hits.append((os.path.basename(f), i + 1, line.strip()))
    assert hits == [], hits


def test_dropout_hash_keeps_every_index_bit_live():
    """the round-3 hash kept 24 bits of state, so a 167,936 x 512 tensor re-used whole rows of masks.  The numpy emulation
    of csrc/common.cuh::dropout_quad (tools/dropout_hash_check.py) at the bench's tensor size: no two rows share a mask, the drop
    rate and the correlations (neighbours, rows, the 2^22 / 2^24-quad lags, key bits) are those of independent draws; the emulation of
    the superseded form must FAIL the same structural test (so the test is known to see the defect)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dropout_hash_check as dh
    cu = open(os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc", "common.cuh")).read()
    for const in ("0xB5297Bu", "0x9E3779u", "0x8DA6B5u", "0x3C6EF3u", "x >> 24", "x >> 15", "x >> 13", "x >> 11"):
        assert const in cu[cu.index("uint2 dropout_quad("):cu.index("dropout_pair(")], const      # the emulation follows the kernel source
    s = dh.structural(dh.quad, 167936)
    assert s["duplicate_row_masks"] == 0 and s["duplicate_quad_frac"] < 0.01, s
    assert dh.structural(dh.quad_r3, 167936)["duplicate_row_masks"] > 30000
    st = dh.statistics(dh.quad, n=1 << 20)
    assert all(abs(r - 0.0635) < 1.5e-3 for r in st["rates"]), st
    assert st["cross_draw_worst"] < 6e-3 and st["key_bit_worst"] < 8e-3 and max(st["lag_worst"].values()) < 6e-3, st
