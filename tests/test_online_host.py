"""CPU checks of the online decoder (contrastiveprosthetics_amd/online.py, csrc/online.cuh): the C ABI of the cp_online_*
entries, the workspace query, and the emission arithmetic -- which windows a chunking emits, and when -- restated against
the CPU oracle of the offline preprocessing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ONLINE = ["cp_online_workspace_bytes", "cp_online_prepare", "cp_online_set_classes", "cp_online_push", "cp_online_reset"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_online_symbols_exported_and_declared(lib):
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in ONLINE:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    body = hdr[hdr.index("typedef struct cp_online_config {"):hdr.index("} cp_online_config;")]
    fields = re.findall(r"\b(\w+)(?:\[\d+\])?\s*[;,]", body)
    assert fields == [f[0] for f in _lib.cp_online_config._fields_], fields
    assert ctypes.sizeof(_lib.cp_online_config) == 6 * 4 + 2 * 17 * 8
    for name in ("MAX_CLASSES", "MAX_VOTE", "MAX_WINDOWS", "STRIDE"):
        v = int(re.search(r"#define CP_ONLINE_%s (\d+)" % name, hdr).group(1))
        assert getattr(_lib, "CP_ONLINE_" + name) == v, name


def test_online_workspace_grows_with_windows_per_push(lib):
    from contrastiveprosthetics_amd._lib import CP_BF16, CP_F32
    for dt in (CP_F32, CP_BF16):
        sizes = [lib.cp_online_workspace_bytes(m, dt) for m in (1, 16, 17, 256, 1024)]
        assert sizes[0] == sizes[1] < sizes[2] < sizes[3] < sizes[4], sizes      # whole 16-row tiles
        assert sizes[0] > 4 * 1000 * 1000 // (2 if dt == CP_BF16 else 1)           # the folded weights live there too
    assert lib.cp_online_workspace_bytes(256, CP_F32) > lib.cp_online_workspace_bytes(256, CP_BF16)


def test_online_entries_refuse_bad_configs(lib):
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_config()
    cfg.dtype, cfg.max_windows, cfg.vote, cfg.phase, cfg.n_coef = _lib.CP_FP8, 16, 25, 0, 9
    cfg.a[0] = 1.0
    buf = ctypes.create_string_buffer(1 << 12)
    assert lib.cp_online_reset(ctypes.byref(cfg), buf, 1 << 12, None) == 10001
    assert b"dtype" in lib.cp_last_error()
    cfg.dtype = _lib.CP_F32
    # AdaBN: no running statistics -> refused before anything is enqueued
    p = _lib.cp_params()
    assert lib.cp_online_prepare(ctypes.byref(cfg), ctypes.byref(p), None, 1e-5, buf, 1 << 12, None) != 0


def _rms_series(rec: np.ndarray) -> np.ndarray:
    """the normalised-before RMS series of a whole recording, positions 0 .. L-11 (moving_rms's [edge:-edge] slice)"""
    from oracle import preprocess_cpu as pc
    b, a = pc.butter_bandpass()
    y = pc.lfilter_df2t(b, a, rec * np.float32(pc.GAIN)).astype(np.float32)
    return np.sqrt(pc.uniform_filter1d_nearest(np.square(y), pc.RMS_WINDOW))[pc.WINDOW_EDGE:-pc.WINDOW_EDGE]


@pytest.mark.parametrize("phase", [0, 13])
def test_emission_arithmetic_against_the_offline_oracle(phase):
    """Window k sits at RMS position phase + 20 k and is emitted by the push that brings raw sample phase + 20 k + 10: its value
    from the samples seen so far equals its value from the whole recording, and the next window is not yet in the series."""
    from contrastiveprosthetics_amd.online import windows_before, windows_emitted
    from oracle import preprocess_cpu as pc
    rng = np.random.default_rng(5 + phase)
    L = 700
    rec = (rng.standard_normal((L, 12)) * 1e-3).astype(np.float32)
    full = _rms_series(rec)
    K = windows_before(L, phase)
    assert K == len(range(phase, L - 10, 20))
    for chunks in ([L], [1] * L, [7] * 100, [20] * 35, [333, 333, 34], list(rng.integers(1, 60, 40))):
        seen, emitted = 0, []
        for n in chunks:
            n = int(min(n, L - seen))
            if n <= 0:
                break
            m = windows_emitted(seen, n, phase)
            first = windows_before(seen, phase)
            seen += n
            prefix = _rms_series(rec[:seen]) if m else None
            for k in range(first, first + m):
                pos = phase + 20 * k
                assert pos + 10 <= seen - 1 < pos + 10 + n                       # final in this push, not before
                assert np.array_equal(prefix[pos], full[pos])
                emitted.append(k)
            nxt = phase + 20 * (first + m)
            assert nxt > seen - 11                                                  # the next one needs more samples
        assert emitted == list(range(K)), chunks
    # and the positions are those of the offline slice: preprocess_segment's first 13 kept rows (time_mask 0, 20, .., 240)
    if phase == 0:
        seg = (rng.standard_normal((pc.SEGMENT_LEN, 12)) * 1e-3).astype(np.float32)
        off = pc.preprocess_segment(seg)
        ser = _rms_series(seg)
        assert np.array_equal(off[:13], ser[20 * np.arange(13)])
