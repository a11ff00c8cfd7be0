"""Class enrolment without a device (contrastiveprosthetics_amd/online.py, include/cpnative.h cp_online_*enroll*): the window
label rule against a brute-force loop, the refusals of `enroll` that need no device, and the argument validation of the C
entries (CP_ERR_ARG and a cp_last_error that names the entry, before anything is enqueued)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
CP_ERR_ARG = 10001


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def _brute(labels, phase):
    out, k = [], 0
    while phase + 20 * k + 10 < len(labels):                   # window k is final once raw sample phase + 20 k + 10 exists
        span = labels[phase + 20 * k: phase + 20 * k + 11]
        out.append(int(span[0]) if span[0] >= 0 and all(v == span[0] for v in span) else -1)
        k += 1
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("phase", [0, 13])
def test_window_labels_against_a_brute_force_loop(phase):
    from contrastiveprosthetics_amd.online import window_labels, windows_before
    n = 1000
    # label changes on the first sample of a window's span, just before it, just after it, on its last sample and behind it
    for k in (3, 17, 30):
        first = phase + 20 * k
        for change in (first - 1, first, first + 1, first + 9, first + 10, first + 11):
            lab = np.full(n, 4, dtype=np.int64)
            lab[change:] = 9
            got = window_labels(lab, phase)
            assert got.shape == (windows_before(n, phase),)
            assert np.array_equal(got, _brute(lab, phase)), (k, change)
            inside = first < change <= first + 10                   # the span holds both labels
            assert got[k] == (-1 if inside else (9 if change <= first else 4)), (k, change)
    # a single unlabelled sample inside a span drops the window, outside it does not
    lab = np.full(n, 2, dtype=np.int64)
    lab[phase + 20 * 5 + 10] = -1
    lab[phase + 20 * 8 + 11] = -1
    got = window_labels(lab, phase)
    assert got[5] == -1 and got[8] == 2 and np.array_equal(got, _brute(lab, phase))
    # seeded cue blocks with unlabelled gaps, every length near a window boundary
    rng = np.random.default_rng(phase)
    for n in (0, 5, phase + 10, phase + 11, phase + 30, phase + 31, 777):
        lab = np.full(n, -1, dtype=np.int32)
        s = 0
        while s < n:
            m = int(rng.integers(1, 90))
            lab[s:s + m] = int(rng.integers(-1, 41))
            s += m
        assert np.array_equal(window_labels(lab, phase), _brute(lab, phase)), n
    assert np.array_equal(window_labels(torch.full((100,), 7, dtype=torch.int32).numpy(), phase), _brute(np.full(100, 7), phase))
    with pytest.raises(ValueError, match="integer"):
        window_labels(np.zeros(100, dtype=np.float32), phase)
    with pytest.raises(ValueError, match="1-d"):
        window_labels(np.zeros((10, 2), dtype=np.int64), phase)
    with pytest.raises(ValueError, match="phase"):
        window_labels(np.zeros(100, dtype=np.int64), 20)


class _Stub:
    """What `_EnrollMixin._enroll` reads of a decoder before it enqueues anything; every device step raises."""
    phase = 0
    device = "cpu"

    def __init__(self, ids=(1, 2, 3), calibrated=True):
        self._enroll_rec = {}
        self._ids = None if ids is None else np.array(ids, dtype=np.int64)
        self._calibrated = calibrated

    def _enroll_view(self, key):
        return self._ids, None, self._calibrated

    def __getattr__(self, name):
        raise AssertionError(f"a refused enroll() reached the device step {name}")


class _CudaLike(torch.Tensor):
    """an (n, 12) f32 tensor that reports a GPU device, so the refusals behind the check of raw can be reached without one"""

    @property
    def device(self):
        return torch.device("cuda:0")


def _raw(n):
    return torch.zeros(n, 12).as_subclass(_CudaLike)


def test_enroll_refusals_that_need_no_device():
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import _EnrollMixin
    call = _EnrollMixin._enroll
    n = 2000
    lab = np.full(n, -1, dtype=np.int64)
    lab[100:900] = 2
    with pytest.raises(_lib.CpNativeError, match="set_classes"):
        call(_Stub(ids=None), None, _raw(n), lab, 1.0, 25, False, False)
    with pytest.raises(_lib.CpNativeError, match="calibrate"):
        call(_Stub(calibrated=False), None, _raw(n), lab, 1.0, 25, False, False)
    for mix in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="mix"):
            call(_Stub(), None, _raw(n), lab, mix, 25, False, False)
    with pytest.raises(ValueError, match="min_windows"):
        call(_Stub(), None, _raw(n), lab, 1.0, 0, False, False)
    with pytest.raises(ValueError, match="raw"):
        call(_Stub(), None, torch.zeros(n, 12), lab, 1.0, 25, False, False)              # not on the GPU
    with pytest.raises(ValueError, match="one entry per raw sample"):
        call(_Stub(), None, _raw(n), lab[:-1], 1.0, 25, False, False)
    with pytest.raises(ValueError, match="integers"):
        call(_Stub(), None, _raw(n), lab.astype(np.float32), 1.0, 25, False, False)
    with pytest.raises(ValueError, match="integers"):
        call(_Stub(), None, _raw(n), torch.zeros(n), 1.0, 25, False, False)
    with pytest.raises(ValueError, match="no labelled window"):
        call(_Stub(), None, _raw(n), np.full(n, -1, dtype=np.int64), 1.0, 25, False, False)
    short = np.full(n, -1, dtype=np.int64)
    short[100:110] = 2                                           # ten samples in a row: no window's 11 fit
    with pytest.raises(ValueError, match="no labelled window"):
        call(_Stub(), None, _raw(n), short, 1.0, 25, False, False)
    other = lab.copy()
    other[1000:1500] = 7
    with pytest.raises(ValueError, match=r"does not have: \[7\]"):
        call(_Stub(), None, _raw(n), other, 1.0, 25, False, False)
    with pytest.raises(ValueError, match="fewer than min_windows"):                         # 500 samples: 24 or 25 windows
        call(_Stub(), None, _raw(n), other, 1.0, 30, True, False)
    with pytest.raises(ValueError, match="at most 64"):
        many = np.repeat(np.arange(100, 166), 30)
        call(_Stub(), None, _raw(many.shape[0]), many, 1.0, 1, True, False)


def _cfg():
    from contrastiveprosthetics_amd import online
    b, a = online._filter(None, None)
    return online._config("f32", 256, 25, 0, b, a)


def test_c_entries_validate_before_anything_is_enqueued(lib):
    """every pointer below is a made-up, suitably aligned address: a call that got past validation would fault or fail with
    a HIP error, not return CP_ERR_ARG"""
    cfg = _cfg()
    P, n = 1 << 20, 100                                          # a 256-byte aligned, non-NULL address

    def refused(rc, entry):
        assert rc == CP_ERR_ARG, (entry, rc, lib.cp_last_error())
        assert entry.encode() in lib.cp_last_error(), (entry, lib.cp_last_error())

    assert lib.cp_online_frontend_state_bytes() % 256 == 0 and 0 < lib.cp_online_frontend_state_bytes() < 8192
    sb = lib.cp_online_frontend_state_bytes()
    refused(lib.cp_online_windows(None, P, sb, P, n, P, P, None), "cp_online_windows")
    refused(lib.cp_online_windows(C.byref(cfg), None, sb, P, n, P, P, None), "cp_online_windows")
    refused(lib.cp_online_windows(C.byref(cfg), P, sb - 1, P, n, P, P, None), "cp_online_windows")
    refused(lib.cp_online_windows(C.byref(cfg), P, sb, P, 20 * 256 + 1, P, P, None), "cp_online_windows")
    refused(lib.cp_online_windows(C.byref(cfg), P, sb, P, -1, P, P, None), "cp_online_windows")
    refused(lib.cp_online_windows(C.byref(cfg), P, sb, None, n, P, P, None), "cp_online_windows")
    refused(lib.cp_online_windows(C.byref(cfg), P, sb, P, n, P, None, None), "cp_online_windows")
    refused(lib.cp_online_windows(C.byref(cfg), P, sb, P + 2, n, P, P, None), "cp_online_windows")

    s1, s256, s999 = (lib.cp_online_enroll_scratch_bytes(k, 0) for k in (1, 256, 999))
    assert 0 < s1 < s256 == s999 and lib.cp_online_enroll_scratch_bytes(999, 1) < s999      # one chunk of <= 256 windows
    assert lib.cp_online_enroll_scratch_bytes(0, 0) == s1
    big = 1 << 40
    single = lambda fn: (lambda w, nw, sl, k, acc, sc, scb: fn(C.byref(cfg), P, big, w, nw, sl, k, acc, sc, scb, None))
    entries = {
        "cp_online_enroll": single(lib.cp_online_enroll),
        "cp_online_adapt_enroll": single(lib.cp_online_adapt_enroll),
        "cp_online_multi_enroll": lambda w, nw, sl, k, acc, sc, scb: lib.cp_online_multi_enroll(
            C.byref(cfg), 4, 512, P, big, w, nw, sl, k, acc, sc, scb, None),
        "cp_online_multi_adapt_enroll": lambda w, nw, sl, k, acc, sc, scb: lib.cp_online_multi_adapt_enroll(
            C.byref(cfg), 4, 512, P, big, 1, w, nw, sl, k, acc, sc, scb, None),
    }
    for name, fn in entries.items():
        refused(fn(P, -1, P, 41, P, P, big), name)
        refused(fn(P, (1 << 24) + 1, P, 41, P, P, big), name)
        refused(fn(P, n, P, 0, P, P, big), name)
        refused(fn(P, n, P, 65, P, P, big), name)
        refused(fn(P, n, P, 41, None, P, big), name)
        refused(fn(P, n, P, 41, P + 4, P, big), name)            # acc holds float64
        refused(fn(None, n, P, 41, P, P, big), name)
        refused(fn(P, n, None, 41, P, P, big), name)
        refused(fn(P, n, P, 41, P, None, big), name)
        refused(fn(P, n, P, 41, P, P + 64, big), name)
        rc = fn(P, n, P, 41, P, P, lib.cp_online_enroll_scratch_bytes(n, 0) - 1)
        assert rc != 0 and b"scratch too small" in lib.cp_last_error() and name.encode() in lib.cp_last_error()
        assert fn(None, 0, None, 41, P, None, 0) == 0            # an empty call is valid and enqueues nothing
    refused(lib.cp_online_multi_adapt_enroll(C.byref(cfg), 4, 512, P, big, 4, P, n, P, 41, P, P, big, None),
            "cp_online_multi_adapt_enroll")
    refused(lib.cp_online_multi_adapt_enroll(C.byref(cfg), 4, 512, P, big, -1, P, n, P, 41, P, P, big, None),
            "cp_online_multi_adapt_enroll")
    assert lib.cp_online_enroll(C.byref(cfg), P, 16, P, n, P, 41, P, P, big, None) != 0      # workspace too small
    assert lib.cp_online_enroll(None, P, big, P, n, P, 41, P, P, big, None) == CP_ERR_ARG

    table = lambda acc, k, prior, mix, mw, out: lib.cp_online_enroll_table(acc, k, prior, C.c_double(mix), mw, out, None)
    for args in ((None, 41, P, 1.0, 25, P), (P, 41, None, 1.0, 25, P), (P, 41, P, 1.0, 25, None), (P, 0, P, 1.0, 25, P),
                 (P, 65, P, 1.0, 25, P), (P, 41, P, -0.01, 25, P), (P, 41, P, 1.01, 25, P), (P, 41, P, float("nan"), 25, P),
                 (P, 41, P, 1.0, 0, P), (P + 4, 41, P, 1.0, 25, P), (P, 41, P + 1, 1.0, 25, P)):
        refused(table(*args), "cp_online_enroll_table")


def test_enrolment_is_exported_from_the_package():
    import contrastiveprosthetics_amd as cp
    from contrastiveprosthetics_amd import online
    assert cp.window_labels is online.window_labels and cp.recording_windows is online.recording_windows
    for cls in (cp.OnlineDecoder, cp.MultiStreamDecoder, cp.AdaptiveMultiStreamDecoder):
        for method in ("enroll", "enroll_reset", "class_table"):
            assert callable(getattr(cls, method))
