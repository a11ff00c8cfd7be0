"""The L2 regulariser + the two Adam optimisers on their own, in torch float64 (CPU or device): what csrc/optim.cuh computes from
four flat buffers and a tensor table, with the semantics of code/models.py:344-349, 467-472 (the regulariser: a sum of Frobenius
norms, NOT squared) and code/train.py:72-73, 107-108 (two torch.optim.Adam with their own learning rates, no weight decay) -- the
formulas of include/cpnative.h above cp_adam_hyper.

    table           rows (offset, numel, group, l2) into the flat buffers: group 0 = emg_net, 1 = glove_net; l2 = the tensor
                    takes part in the regulariser
    per tensor      n     = |p|                                       (Frobenius norm of the tensor)
                    value = sum over the members of reg[group] * n
    per element     g'    = grad_scale * g  +  reg[group] * p / n     (members only; the second term is 0 where n = 0:
                                                                       torch.norm's gradient at the zero tensor is 0)
                    m'    = beta1 * m + (1 - beta1) * g'
                    v'    = beta2 * v + (1 - beta2) * g'^2
                    p'    = p - (lr[group] / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps)          (torch.optim.Adam, amsgrad off)
    bc1, bc2        1 - beta^t, formed in double and rounded to float32, as the library's host code does; or given

Every hyper-parameter enters as the float32 value the library receives (cp_adam_hyper holds floats), widened.  Elements outside
the table are returned as they came.

`dtype=torch.float32` evaluates the same formulas in plain torch float32, scalars included: the yardstick for a single-precision
kernel's error (tests/test_gpu_optim.py derives its bars from it).

`norms=` takes the per-tensor norms as given instead of forming them (what a kernel does that reads a norm table), for tests
that ask what a wrong norm would do.

Besides p, m, v, the regulariser value and the norms, the result carries the two scales a comparison needs:
    m_scale   beta1 |m| + (1 - beta1) (|grad_scale g| + |reg p / n|): the magnitudes of the terms m' is made of (m' itself can
              cancel to nearly nothing)
    p_scale   (lr / bc1) m_scale / (sqrt(v') / sqrt(bc2) + eps): the same for the update p' - p
and `extent`, the smallest and the largest magnitude of every non-zero intermediate value, for a test that wants subnormals and
overflow out of the picture."""
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

HYPER_KEYS = ("lr_emg", "lr_glove", "reg_emg", "reg_glove", "beta1", "beta2", "eps")


def as_float32(x: float) -> float:
    """the value a float field of the C ABI holds, widened"""
    return float(np.float32(x))


def bias_corrections(beta1: float, beta2: float, step: int) -> Tuple[float, float]:
    """(bc1, bc2) as csrc/api.hip forms them: the float32 betas widened, the power and the difference in double, the result
    rounded to float32"""
    b1, b2 = as_float32(beta1), as_float32(beta2)
    return as_float32(1.0 - b1 ** step), as_float32(1.0 - b2 ** step)


def l2_adam_reference(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                      table: Sequence[Tuple[int, int, int, int]], hyper: Dict[str, float], grad_scale: float = 1.0,
                      step: Optional[int] = None, bc1: Optional[float] = None, bc2: Optional[float] = None,
                      lr_emg: Optional[float] = None, lr_glove: Optional[float] = None,
                      norms: Optional[Sequence[float]] = None, dtype=torch.float64) -> Dict[str, object]:
    """-> p, m, v (flat, as the inputs), l2 (the regulariser value), norms (one per table row), m_scale, p_scale (flat float64,
    0 outside the table), extent (min, max magnitude of the non-zero intermediates).  Either `step` (1-based) or bc1 and bc2;
    lr_emg / lr_glove override hyper's (a scheduled rate, as cp_step_state carries it).  Values given explicitly are used as
    given: the caller rounds them to float32 where a float field of the library is meant."""
    assert (step is None) != (bc1 is None) and (bc1 is None) == (bc2 is None)
    if step is not None:
        assert step >= 1
        bc1, bc2 = bias_corrections(hyper["beta1"], hyper["beta2"], step)
    h = {k: as_float32(hyper[k]) for k in HYPER_KEYS}
    if lr_emg is not None:
        h["lr_emg"] = float(lr_emg)
    if lr_glove is not None:
        h["lr_glove"] = float(lr_glove)
    dev = p.device
    S = lambda x: torch.tensor(float(x), dtype=dtype, device=dev)           # a scalar of the working precision
    lr, reg = (S(h["lr_emg"]), S(h["lr_glove"])), (S(h["reg_emg"]), S(h["reg_glove"]))
    b1, b2, eps, gs = S(h["beta1"]), S(h["beta2"]), S(h["eps"]), S(as_float32(grad_scale))
    one = S(1.0)
    rbc2 = torch.sqrt(S(bc2))
    P, G, M, V = (t.detach().to(dtype).clone() for t in (p, g, m, v))
    m_scale = torch.zeros(P.shape, dtype=torch.float64, device=dev)
    p_scale = torch.zeros(P.shape, dtype=torch.float64, device=dev)
    out_norms = torch.zeros(len(table), dtype=dtype, device=dev)
    value = S(0.0)
    lo, hi = float("inf"), 0.0

    def seen(*tensors):
        nonlocal lo, hi
        for t in tensors:
            a = t.detach().double().abs().reshape(-1)
            a = a[a > 0]
            if a.numel():
                lo, hi = min(lo, float(a.min())), max(hi, float(a.max()))

    for i, (off, numel, group, l2) in enumerate(table):
        sl = slice(off, off + numel)
        x = P[sl]
        n = torch.sqrt((x * x).sum()) if norms is None else S(norms[i])     # (torch.sum adds in a cascade: the float32 mode's norm is good to its last bits)
        out_norms[i] = n
        if numel == 0:
            continue
        step_size = lr[group] / S(bc1)
        data = gs * G[sl]
        if l2:
            value = value + reg[group] * n
            pen = reg[group] / n * x if float(n) > 0 else torch.zeros_like(x)
        else:
            pen = torch.zeros_like(x)
        ge = data + pen
        m_scale[sl] = (b1 * M[sl].abs() + (one - b1) * (data.abs() + pen.abs())).double()
        mn = b1 * M[sl] + (one - b1) * ge
        vn = b2 * V[sl] + (one - b2) * ge * ge
        denom = torch.sqrt(vn) / rbc2 + eps
        upd = step_size * (mn / denom)
        p_scale[sl] = float(step_size) * m_scale[sl] / denom.double()
        seen(x, G[sl], data, pen, ge, ge * ge, M[sl], V[sl], mn, vn, denom, upd, n * n, n, x - upd)
        P[sl], M[sl], V[sl] = x - upd, mn, vn
    return dict(p=P, m=M, v=V, l2=value, norms=out_norms, m_scale=m_scale, p_scale=p_scale, extent=(lo, hi))
