"""Head fine-tuning without a device (contrastiveprosthetics_amd/finetune.py, online.py finetune, include/cpnative.h
cp_online_finetune_*): the float64 restatement against torch autograd and torch.optim.Adam, the fitness of the inputs the GPU
tests use, the refusals of `finetune` that need no device, and the argument validation of the C entries (CP_ERR_ARG and a
cp_last_error that names the entry, before anything is enqueued)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from finetune_problem import synthetic_problem  # noqa: E402  (tests/finetune_problem.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
CP_ERR_ARG = 10001

SHAPES = [(n, k) for n in (1, 17, 130) for k in (2, 41, 64)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def _weights(slots, k, balanced):
    """w_i from the definition, on its own"""
    counts = np.bincount(slots, minlength=k)
    if not balanced:
        return np.full(slots.shape[0], 1.0 / slots.shape[0])
    return 1.0 / ((counts > 0).sum() * counts[slots])


def _torch_objective(u, W, b, E, slots, w, scale, anchor=0.0, start=None):
    z = u @ W.t() + b
    zn = z / z.norm(dim=1, keepdim=True)
    en = E / E.norm(dim=1, keepdim=True)
    l = scale * zn @ en.t()
    loss = (w * (torch.logsumexp(l, dim=1) - l[torch.arange(l.shape[0]), slots])).sum()
    if anchor:
        loss = loss + 0.5 * anchor * sum(((p - p0) ** 2).sum() for p, p0 in zip((W, b, E), start))
    return loss


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("balanced", [True, False])
@pytest.mark.parametrize("n,k", SHAPES)
def test_reference_gradient_against_autograd(n, k, balanced):
    """both sides are float64: 1e-10 of each tensor's largest entry.  Class k-1 has no window in every problem; the second
    step's gradient is taken away from theta_0, where the anchor term is not zero."""
    from contrastiveprosthetics_amd.finetune import finetune_reference
    q = synthetic_problem(n, k, seed=3)
    assert k - 1 not in q["slots"]
    scale, anchor = 3.0, 0.25
    ref = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], steps=2, lr=5e-3, lr_rows=2e-2, scale=scale, anchor=anchor,
                             balanced=balanced)
    T = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    slots = torch.tensor(q["slots"].astype(np.int64))
    w = T(_weights(q["slots"], k, balanced))
    start = [T(q[name]) for name in ("W", "b", "E")]
    for step, at in ((0, start), (1, [T(x) for x in ref["trace"][0]])):
        params = [p.clone().requires_grad_(True) for p in at]
        loss = _torch_objective(T(q["u"]), *params, slots, w, scale, anchor, start)
        loss.backward()
        plain = _torch_objective(T(q["u"]), *at, slots, w, scale)
        assert abs(ref["loss"][step] - float(plain)) <= 1e-10 * abs(float(plain))
        if step == 1:
            for name, got, p in zip(("dW", "db", "dE"), ref["grad"], params):
                assert _rel(got, p.grad.numpy()) <= 1e-10, (name, step)
    first = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], steps=1, scale=scale, anchor=anchor, balanced=balanced)
    params = [p.clone().requires_grad_(True) for p in start]
    _torch_objective(T(q["u"]), *params, slots, w, scale, anchor, start).backward()
    for name, got, p in zip(("dW", "db", "dE"), first["grad"], params):
        assert _rel(got, p.grad.numpy()) <= 1e-10, name
    assert np.abs(first["grad"][2][k - 1]).max() > 0            # a class without windows is still pushed away by the others


@pytest.mark.parametrize("n,k", [(17, 41), (130, 64)])
def test_five_reference_steps_against_torch_adam(n, k):
    from contrastiveprosthetics_amd.finetune import finetune_reference
    q = synthetic_problem(n, k, seed=5)
    scale, anchor, lr, lr_rows = 2.0, 0.1, 3e-3, 1e-2
    ref = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], steps=5, lr=lr, lr_rows=lr_rows, scale=scale, anchor=anchor)
    T = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    start = [T(q[name]) for name in ("W", "b", "E")]
    params = [p.clone().requires_grad_(True) for p in start]
    opt = torch.optim.Adam([dict(params=params[:2], lr=lr), dict(params=params[2:], lr=lr_rows)], betas=(0.9, 0.999), eps=1e-8)
    slots, w = torch.tensor(q["slots"].astype(np.int64)), T(_weights(q["slots"], k, True))
    for _ in range(5):
        opt.zero_grad()
        _torch_objective(T(q["u"]), *params, slots, w, scale, anchor, start).backward()
        opt.step()
    for name, got, p, p0 in zip(("W", "b", "E"), (ref["W"], ref["b"], ref["E"]), params, start):
        moved = float((p.detach() - p0).abs().max())
        assert moved > 1e-3                                      # five steps of about lr each
        assert float(np.abs(got - p.detach().numpy()).max()) <= 1e-10 * float(p.detach().abs().max()), name
    # a tensor that is not trained is returned as it came
    rows_only = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], steps=3, train_projection=False)
    assert np.array_equal(rows_only["W"], q["W"]) and np.array_equal(rows_only["b"], q["b"]) and not np.array_equal(rows_only["E"], q["E"])


@pytest.mark.parametrize("bf16", [False, True])
def test_the_loss_falls_on_the_inputs_the_gpu_tests_use(bf16):
    """20 reference steps at the kernel's rounding points on every shape of tests/test_gpu_online_finetune.py: a problem whose
    loss did not fall would make its comparisons of trained tensors say little"""
    from contrastiveprosthetics_amd.finetune import finetune_reference, round_bf16
    for n in (1, 15, 16, 17, 63, 64, 65, 130):
        for k in (2, 41, 64):
            q = synthetic_problem(n, k, seed=11, bf16=bf16)
            ref = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], steps=21, lr=1e-3, lr_rows=1e-2, scale=4.0,
                                     round_w=round_bf16 if bf16 else None, f32_points=True)
            assert np.isfinite(ref["loss"]).all() and ref["loss"][20] < ref["loss"][0], (n, k)


def test_round_bf16_is_round_to_nearest_even():
    from contrastiveprosthetics_amd.finetune import round_bf16
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3
    x = torch.cat([x, torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895e38])])       # two ties: to even, both ways
    assert np.array_equal(round_bf16(x.numpy()), x.to(torch.bfloat16).double().numpy())


# ----------------------------------------------------------------------------------------------------------------------------
class _Stub:
    """What `_EnrollMixin._finetune` reads of a decoder before it enqueues anything; every device step raises."""
    phase = 0
    device = "cpu"

    def __init__(self, ids=(1, 2, 3), calibrated=True, shared=False):
        self._ids = None if ids is None else np.array(ids, dtype=np.int64)
        self._calibrated = calibrated
        self._shared_projection = shared

    def _enroll_view(self, key):
        return self._ids, None, self._calibrated

    def __getattr__(self, name):
        raise AssertionError(f"a refused finetune() reached the device step {name}")


class _CudaLike(torch.Tensor):
    """an (n, 12) f32 tensor that reports a GPU device, so the refusals behind the check of raw can be reached without one"""

    @property
    def device(self):
        return torch.device("cuda:0")


def _raw(n):
    return torch.zeros(n, 12).as_subclass(_CudaLike)


def test_finetune_refusals_that_need_no_device():
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, MultiStreamDecoder, OnlineDecoder, _EnrollMixin
    assert MultiStreamDecoder._shared_projection and AdaptiveMultiStreamDecoder._shared_projection
    assert not OnlineDecoder._shared_projection

    def call(stub, raw, lab, steps=10, lr=1e-3, lr_rows=None, scale=1.0, anchor=0.0, train_projection=True, min_windows=25):
        return _EnrollMixin._finetune(stub, None, raw, lab, steps, lr, lr_rows, scale, anchor, True, train_projection, True, min_windows,
                                      False)
    n = 2000
    lab = np.full(n, -1, dtype=np.int64)
    lab[100:900] = 2
    with pytest.raises(ValueError, match="shared by all streams"):
        call(_Stub(shared=True), _raw(n), lab)
    with pytest.raises(_lib.CpNativeError, match="set_classes"):
        call(_Stub(ids=None), _raw(n), lab)
    with pytest.raises(_lib.CpNativeError, match="calibrate"):
        call(_Stub(calibrated=False), _raw(n), lab)
    for steps in (-1, 2.5, True):
        with pytest.raises(ValueError, match="steps"):
            call(_Stub(), _raw(n), lab, steps=steps)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lr"):
            call(_Stub(), _raw(n), lab, lr=bad)
        with pytest.raises(ValueError, match="lr_rows"):
            call(_Stub(), _raw(n), lab, lr_rows=bad)
        with pytest.raises(ValueError, match="anchor"):
            call(_Stub(), _raw(n), lab, anchor=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            call(_Stub(), _raw(n), lab, scale=bad)
    with pytest.raises(ValueError, match="min_windows"):
        call(_Stub(), _raw(n), lab, min_windows=0)
    with pytest.raises(ValueError, match="raw"):
        call(_Stub(), torch.zeros(n, 12), lab)                                    # not on the GPU
    with pytest.raises(ValueError, match="one entry per raw sample"):
        call(_Stub(), _raw(n), lab[:-1])
    with pytest.raises(ValueError, match="no labelled window"):
        call(_Stub(), _raw(n), np.full(n, -1, dtype=np.int64))
    other = lab.copy()
    other[1000:1500] = 7
    with pytest.raises(ValueError, match=r"does not have: \[7\]"):                   # an unknown id
        call(_Stub(), _raw(n), other)
    known = lab.copy()
    known[1000:1500] = 3                                                          # 500 samples: 24 or 25 windows
    with pytest.raises(ValueError, match=r"classes \[3\] have fewer than min_windows=30"):
        call(_Stub(), _raw(n), known, min_windows=30)
    # a class without windows (1) is no refusal, and steps = 0 returns the counts without a device call
    assert call(_Stub(), _raw(n), known, steps=0, min_windows=20) == {1: 0, 2: 40, 3: 25}


def _cfg(dtype="f32"):
    from contrastiveprosthetics_amd import online
    b, a = online._filter(None, None)
    return online._config(dtype, 256, 25, 0, b, a)


def test_c_entries_validate_before_anything_is_enqueued(lib):
    """every pointer below is a made-up, suitably aligned address: a call that got past validation would fault or fail with
    a HIP error, not return CP_ERR_ARG"""
    cfg = _cfg()
    P, n, k = 1 << 20, 100, 41
    nan, inf = float("nan"), float("inf")

    def refused(rc, entry, code=CP_ERR_ARG):
        assert (rc == code if code else rc != 0), (entry, rc, lib.cp_last_error())
        assert entry.encode() in lib.cp_last_error() or b"cp_online" in lib.cp_last_error(), (entry, lib.cp_last_error())

    # ---- the state
    sb = lib.cp_online_finetune_state_bytes(n, k)
    assert sb % 256 == 0 and lib.cp_online_finetune_state_bytes(64, k) < lib.cp_online_finetune_state_bytes(65, k)     # one more slab
    assert lib.cp_online_finetune_state_bytes(0, k) == lib.cp_online_finetune_state_bytes(1, k)
    init = lambda st=P, b=sb, dt=0, W=P, bb=P, E=P, sl=P, nn=n, kk=k, bal=1: lib.cp_online_finetune_init(st, b, dt, W, bb, E, sl, nn, kk, bal,
                                                                                                       None)
    for kw in (dict(st=None), dict(st=P + 128), dict(b=sb - 1), dict(dt=2), dict(W=None), dict(bb=None), dict(E=None), dict(sl=None),
               dict(W=P + 2), dict(nn=0), dict(nn=(1 << 24) + 1), dict(kk=0), dict(kk=65), dict(bal=2)):
        refused(init(**kw), "cp_online_finetune_init")

    def steps(c=C.byref(cfg), st=P, b=sb, u=P, nn=n, kk=k, ns=3, lr=1e-3, lrr=1e-3, sc=1.0, an=0.0, fl=3, lo=P):
        return lib.cp_online_finetune_steps(c, st, b, u, nn, kk, ns, lr, lrr, sc, an, fl, lo, None)
    for kw in (dict(c=None), dict(st=None), dict(st=P + 64), dict(b=sb - 1), dict(u=None), dict(u=P + 8), dict(nn=0), dict(kk=0),
               dict(kk=65), dict(ns=-1), dict(lr=nan), dict(lr=inf), dict(lr=-1.0), dict(lrr=nan), dict(lrr=-1.0), dict(sc=nan),
               dict(sc=inf), dict(sc=1e300), dict(an=nan), dict(an=inf), dict(an=-0.5), dict(fl=4), dict(lo=None), dict(lo=P + 4)):
        refused(steps(**kw), "cp_online_finetune_steps")
    fp8 = _cfg()
    fp8.dtype = 2
    refused(steps(c=C.byref(fp8)), "cp_online_finetune_steps")
    assert steps(ns=0, lo=None) == 0                             # an empty call is valid and enqueues nothing
    read = lambda st=P, b=sb, nn=n, kk=k, W=P, bb=P, E=P, g=None: lib.cp_online_finetune_read(st, b, nn, kk, W, bb, E, g, None)
    for kw in (dict(st=None), dict(b=sb - 1), dict(kk=65), dict(W=None), dict(bb=None), dict(E=None), dict(g=P + 4), dict(nn=-1)):
        refused(read(**kw), "cp_online_finetune_read")

    # ---- the tail inputs: the enrol chain's checks, out 16-byte aligned, and the form of the workspace
    ws_f, ws_a = lib.cp_online_workspace_bytes(256, 0), lib.cp_online_adapt_workspace_bytes(256, 0)
    wm_f, wm_a = lib.cp_online_multi_workspace_bytes(4, 512, 0), lib.cp_online_multi_adapt_workspace_bytes(4, 512, 0)
    assert ws_f < ws_a and wm_f < wm_a
    # the forms are told apart by their sizes: an adaptive workspace is the larger one for every configuration
    for dt in (0, 1):
        for mw in (1, 15, 16, 255, 256):
            assert lib.cp_online_workspace_bytes(mw, dt) < lib.cp_online_adapt_workspace_bytes(mw, dt)
        for s, rows in ((1, 1), (1, 256), (3, 17), (64, 4096), (256, 65536)):
            assert lib.cp_online_multi_workspace_bytes(s, rows, dt) < lib.cp_online_multi_adapt_workspace_bytes(s, rows, dt)
    big = 1 << 40
    entries = {
        "cp_online_tail_inputs": lambda w, nw, out, sc, scb, wsb=ws_f: lib.cp_online_tail_inputs(C.byref(cfg), P, wsb, w, nw, out, sc, scb, None),
        "cp_online_adapt_tail_inputs": lambda w, nw, out, sc, scb, wsb=ws_a: lib.cp_online_adapt_tail_inputs(
            C.byref(cfg), P, wsb, w, nw, out, sc, scb, None),
        "cp_online_multi_tail_inputs": lambda w, nw, out, sc, scb, wsb=wm_f: lib.cp_online_multi_tail_inputs(
            C.byref(cfg), 4, 512, P, wsb, w, nw, out, sc, scb, None),
        "cp_online_multi_adapt_tail_inputs": lambda w, nw, out, sc, scb, wsb=wm_a: lib.cp_online_multi_adapt_tail_inputs(
            C.byref(cfg), 4, 512, P, wsb, 1, w, nw, out, sc, scb, None),
    }
    other_form = {"cp_online_tail_inputs": ws_a, "cp_online_adapt_tail_inputs": ws_f, "cp_online_multi_tail_inputs": wm_a,
                  "cp_online_multi_adapt_tail_inputs": wm_f}
    for name, fn in entries.items():
        refused(fn(P, -1, P, P, big), name)
        refused(fn(P, (1 << 24) + 1, P, P, big), name)
        refused(fn(None, n, P, P, big), name)
        refused(fn(P, n, None, P, big), name)
        refused(fn(P, n, P + 8, P, big), name)                   # rows of out are read 16 bytes at a time
        refused(fn(P, n, P, None, big), name)
        refused(fn(P, n, P, P + 64, big), name)
        refused(fn(P, n, P, P, lib.cp_online_enroll_scratch_bytes(n, 0) - 1), name, code=None)
        assert b"scratch too small" in lib.cp_last_error()
        refused(fn(P, n, P, P, big, other_form[name]), name, code=None)      # a folded entry on an adaptive workspace, and the reverse
        assert fn(None, 0, None, None, 0) == 0
    refused(lib.cp_online_multi_adapt_tail_inputs(C.byref(cfg), 4, 512, P, wm_a, 4, P, n, P, P, big, None), "cp_online_multi_adapt_tail_inputs")

    # ---- the projection
    for name, wsb, other in (("cp_online_set_projection", ws_f, ws_a), ("cp_online_adapt_set_projection", ws_a, ws_f),
                             ("cp_online_projection", ws_f, ws_a), ("cp_online_adapt_projection", ws_a, ws_f)):
        fn = getattr(lib, name)
        refused(fn(None, P, wsb, P, P, None), name)
        refused(fn(C.byref(cfg), None, wsb, P, P, None), name)
        refused(fn(C.byref(cfg), P, wsb, None, P, None), name)
        refused(fn(C.byref(cfg), P, wsb, P, None, None), name)
        refused(fn(C.byref(cfg), P, wsb, P + 2, P, None), name)
        refused(fn(C.byref(cfg), P, other, P, P, None), name, code=None)
        refused(fn(C.byref(cfg), P, wsb + 256, P, P, None), name, code=None)
    for name, wsb, other in (("cp_online_multi_projection", wm_f, wm_a), ("cp_online_multi_adapt_projection", wm_a, wm_f)):
        fn = getattr(lib, name)
        refused(fn(C.byref(cfg), 4, 512, P, wsb, None, P, None), name)
        refused(fn(C.byref(cfg), 4, 512, P, other, P, P, None), name, code=None)
        refused(fn(C.byref(cfg), 0, 512, P, wsb, P, P, None), name)


def test_finetuning_is_exported_and_the_constants_agree():
    import re
    import contrastiveprosthetics_amd as cp
    from contrastiveprosthetics_amd import _lib, finetune
    assert cp.finetune_reference is finetune.finetune_reference
    for method in ("finetune", "projection", "set_projection", "reset_projection"):
        assert callable(getattr(cp.OnlineDecoder, method))
    for cls in (cp.MultiStreamDecoder, cp.AdaptiveMultiStreamDecoder):
        assert callable(cls.finetune)
    hdr = open(os.path.join(ROOT, "include", "cpnative.h")).read()
    for name in ("CP_ONLINE_FINETUNE_CHUNK", "CP_ONLINE_FINETUNE_PROJECTION", "CP_ONLINE_FINETUNE_ROWS"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, name)
