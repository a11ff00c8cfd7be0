"""Head fine-tuning restated in numpy float64: the definition `OnlineDecoder.finetune` is held to (include/cpnative.h,
"head fine-tuning"; csrc/online_finetune.cuh).  Host only.

The trained numbers are the projection W (16, 512) with its bias b (16) and the class rows E (K, 16); the data are the tail
inputs u (N, 512) of the labelled windows and their slots y.  With W_T the master W as the forward sees it,

    z_i = W_T u_i + b        z^_i = z_i / |z_i|        E^_c = E_c / |E_c|        l_ic = scale z^_i . E^_c
    L = sum_i w_i (-log softmax_c(l_i)[y_i])           w_i = 1 / (C n_{y_i})  (balanced)  or  1 / N
    g_ic = w_i scale (p_ic - [c = y_i])                dz^_i = sum_c g_ic E^_c
    dz_i = (dz^_i - z^_i (z^_i . dz^_i)) / |z_i|       dW = sum_i dz_i u_i^T        db = sum_i dz_i
    dE^_c = sum_i g_ic z^_i                            dE_c = (dE^_c - E^_c (E^_c . dE^_c)) / |E_c|
    every trained tensor: + anchor (theta - theta_0)   then Adam (beta 0.9 / 0.999, eps 1e-8, bias-corrected)

The device rounds at a few points, and the reference takes them as arguments so that a comparison is held to the arithmetic
and not to the formats: `u` enters as stored (the caller passes the stored values widened), `round_w` maps the master W to W_T
(`round_bf16` for a bf16 decoder, None for f32), and `f32_points=True` forms z^, E^, w_i and the stored masters and moments
in float32 as the kernels do (z^ and E^ operation for operation).  With f32_points=False and round_w=None everything is
float64: that is the form the autograd check differentiates.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def round_bf16(x) -> np.ndarray:
    """x rounded to bfloat16 (round to nearest even) and widened again, as float64"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def _unit_rows(x: np.ndarray, f32: bool):
    """rows / |row| and |row|: float64, or float32 with the 16 squares summed in order as the kernels sum them"""
    if not f32:
        n = np.sqrt((x * x).sum(axis=1))
        return x / n[:, None], n
    x32 = x.astype(np.float32)
    ss = np.zeros(x.shape[0], dtype=np.float32)
    for d in range(x.shape[1]):
        ss = ss + x32[:, d] * x32[:, d]
    n = np.sqrt(ss)
    return (x32 / n[:, None]).astype(np.float64), n.astype(np.float64)


def class_weights(slots, n_classes: int, balanced: bool = True, f32: bool = False) -> np.ndarray:
    """w_i of every window; a window whose slot lies outside 0..n_classes-1 weighs nothing"""
    y = np.asarray(slots, dtype=np.int64)
    ok = (y >= 0) & (y < n_classes)
    counts = np.bincount(y[ok], minlength=n_classes).astype(np.float64)
    per = np.zeros(n_classes)
    has = counts > 0
    per[has] = 1.0 / (has.sum() * counts[has]) if balanced else 1.0 / counts.sum()
    if f32:
        per = per.astype(np.float32).astype(np.float64)
    w = np.zeros(y.shape[0])
    w[ok] = per[y[ok]]
    return w


def loss_and_gradient(u, W, b, E, slots, *, scale: float = 1.0, balanced: bool = True, round_w: Optional[Callable] = None,
                      f32_points: bool = False, normalisation_backward: bool = True):
    """L and (dW, db, dE) at (W, b, E), without the anchor.  normalisation_backward=False leaves the z^ (z^ . dz^) term
    out of dz: a deliberately wrong backward that a test's tolerance must be able to tell from the right one."""
    u = np.asarray(u, dtype=np.float64)
    W, b, E = (np.asarray(t, dtype=np.float64) for t in (W, b, E))
    y = np.asarray(slots, dtype=np.int64)
    K = E.shape[0]
    w = class_weights(y, K, balanced, f32_points)
    Wt = W if round_w is None else np.asarray(round_w(W), dtype=np.float64)
    z = u @ Wt.T + b
    if f32_points:
        z = z.astype(np.float32).astype(np.float64)
    zn, zlen = _unit_rows(z, f32_points)
    en, elen = _unit_rows(E, f32_points)
    l = scale * (zn @ en.T)
    l = l - l.max(axis=1, keepdims=True)
    ex = np.exp(l)
    se = ex.sum(axis=1, keepdims=True)
    p = ex / se
    live = w > 0
    ys = np.where(live, y, 0)
    rows = np.arange(y.shape[0])
    nll = np.log(se[:, 0]) - l[rows, ys]
    L = float((w[live] * nll[live]).sum())
    g = p.copy()
    g[rows, ys] -= 1.0
    g *= (w * scale)[:, None]
    dzn = g @ en
    dz = dzn - zn * (zn * dzn).sum(axis=1, keepdims=True) if normalisation_backward else dzn
    dz = dz / zlen[:, None]
    dz[~live] = 0.0
    den = g[live].T @ zn[live]
    dE = (den - en * (en * den).sum(axis=1, keepdims=True)) / elen[:, None]
    return L, (dz.T @ u, dz.sum(axis=0), dE)


def finetune_reference(u, W, b, E, slots, *, steps: int = 1, lr: float = 1e-3, lr_rows: Optional[float] = None, scale: float = 1.0,
                       anchor: float = 0.0, balanced: bool = True, train_projection: bool = True, train_rows: bool = True,
                       round_w: Optional[Callable] = None, f32_points: bool = False, normalisation_backward: bool = True) -> dict:
    """`steps` Adam steps from (W, b, E).  Returns W, b, E (float64 arrays; float32 values under f32_points), loss (steps,) --
    L of each step before its update -- grad = (dW, db, dE) of the last step with the anchor term, and trace: (W, b, E)
    after every step."""
    theta = [np.array(t, dtype=np.float64) for t in (W, b, E)]
    if f32_points:
        theta = [t.astype(np.float32).astype(np.float64) for t in theta]
    theta0 = [t.copy() for t in theta]
    m = [np.zeros_like(t) for t in theta]
    v = [np.zeros_like(t) for t in theta]
    rates = (lr, lr, lr if lr_rows is None else lr_rows)
    trained = (train_projection, train_projection, train_rows)
    keep = (lambda x: x.astype(np.float32).astype(np.float64)) if f32_points else (lambda x: x)
    loss, trace, grad = [], [], None
    for t in range(1, int(steps) + 1):
        L, grad = loss_and_gradient(u, *theta, slots, scale=scale, balanced=balanced, round_w=round_w, f32_points=f32_points,
                                    normalisation_backward=normalisation_backward)
        grad = tuple(g + anchor * (p - p0) for g, p, p0 in zip(grad, theta, theta0))
        loss.append(L)
        bc1, bc2 = 1.0 - BETA1 ** t, 1.0 - BETA2 ** t
        for i in range(3):
            if not trained[i]:
                continue
            m[i] = keep(BETA1 * m[i] + (1.0 - BETA1) * grad[i])
            v[i] = keep(BETA2 * v[i] + (1.0 - BETA2) * grad[i] * grad[i])
            theta[i] = keep(theta[i] - (rates[i] / bc1) * (m[i] / (np.sqrt(v[i]) / np.sqrt(bc2) + EPS)))
        trace.append(tuple(p.copy() for p in theta))
    return dict(W=theta[0], b=theta[1], E=theta[2], loss=np.array(loss), grad=grad, trace=trace)
