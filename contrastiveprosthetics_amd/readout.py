"""Closed-form head fit: ridge projection onto the class rows, without a gradient.

A user's own projection (16 x 512 + 16) could only come from `finetune`, a gradient run with a learning rate, a step count, a
scale and an anchor.  This module fits it in closed form: the tail inputs u of a user's cued recording are regressed onto the
unit class rows the decoder already has, with a ridge penalty, by the normal equations.  One knob (the ridge), deterministic,
and cheap enough to be scored per ridge value on repetitions it has not seen (`pick_ridge`).  The device side is
cp_online_readout_moments / _solve / _apply (include/cpnative.h, csrc/online_readout.cuh); `fit_reference` and
`apply_reference` are the definitions, in numpy float64 with every operation rounded on its own (no fused multiply-add, no
BLAS, no np.linalg).  The device's moments and solve equal them in every bit.

Inputs.  u (N, 512): the tail inputs as stored (f32 or bf16 values, widened exactly); x_i = [u_i, 1] (513 values).  slot y_i in
0..K-1 (K <= 64), negative: the window is not used.  group (repetition) r_i in 0..R-1, R <= 16, negative: not used.  weight w_i,
float64, from the host (`window_weights`): balanced 1 / (C n_{y_i}) over all used windows, C the slots with windows, else
1 / N_used.  These weights sum to 1 over the recording; a plan that trains on a subset of the groups simply carries less
weight (its ridge is that much stronger relative to the data).  targets E^ (K, 16) f32: the unit class rows exactly as
`set_classes` normalises them (`unit_targets`).

Moments per group, over its used windows in recording order, every element from 0:
G_r[a][b] += w_i * (x_ia * x_ib) and C_r[a][d] += w_i * (x_ia * E^[y_i][d]).  The inner product of two f32 values is exact in
float64; then one rounded multiply by w_i and one rounded add.  Each element's sum is strictly sequential in window order.

Plans.  A plan is (group mask, ridge >= 0).  A = the sum of G_r over the mask in ascending r, from 0, + ridge * D with D the
identity except D[512][512] = 0 (the bias is not penalised); B = the sum of C_r in the same order.

Cholesky A = L L^T in float64: element (i, j) starts from A[i][j] and has L[i][k] * L[j][k] subtracted for k = 0..j-1 in
ascending k, one rounded multiply and one rounded subtract each, then sqrt (i == j) or the division by L[j][j].  A pivot that
is not finite or not > 0 at column j gives the plan status = j + 1 and zero W and b; nothing else of that plan is defined.

Solve.  Forward substitution y[a] = (B[a] - sum over k = 0..a-1 ascending of L[a][k] * y[k]) / L[a][a]; backward substitution
x[a] = (y[a] - sum over k = a+1..512 ascending of L[k][a] * x[k]) / L[a][a]; both for the 16 right-hand sides, every product
and every subtraction rounded on its own.  W[d][a] = float32(x[a][d]), b[d] = float32(x[512][d]).

Apply.  z_i = W_T u_i + b with W rounded to the decoder's compute dtype, multiplied and summed as the tail of a push does:
wave w of eight sums the 32-wide chunks w and w + 8 of the 512 products in f32, one matrix instruction per 4 (f32) or 32
(bf16) products, the eight partial sums are added in wave order, then the bias; z^_i = z_i / sqrtf(sum of z^2) in f32, the squares
summed in order.  The device runs the push tail's own tile code, so `Readout.apply` is bit for bit what a push with
`set_projection(W, b)` installed emits as its embedding.  The order inside one matrix instruction is not documented.
`apply_reference` takes what the MI355X was measured to do in f32: one fused multiply-add per product, the four products of an
instruction in ascending k; with that it equals the device in every bit for an f32 decoder.  For bf16 it adds an instruction's
32 products as four partial sums of 8, the closest order found (about 1 element in 70 still differs in its last bit), so a bf16
table is scored from the device's apply.

Nothing here is about real subjects; `readout_recording` is a synthetic person.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from . import holdout as H
from .finetune import round_bf16
from .track import _expected_slots, _host, _ids_array

REST, IGNORE = -1, -2                   # online.REST, online.IGNORE
D_E = _lib.CP_D_E
F = 512                                 # tail inputs per window
X = _lib.CP_ONLINE_READOUT_X            # x = [u, 1]
MAX_CLASSES = _lib.CP_ONLINE_MAX_CLASSES
MAX_GROUPS = _lib.CP_ONLINE_READOUT_MAX_GROUPS
MAX_PLANS = _lib.CP_ONLINE_READOUT_MAX_PLANS
STAGE = _lib.CP_ONLINE_READOUT_STAGE    # windows the moments kernel stages at a time
RIDGES = (1e-3, 1e-2, 1e-1, 1.0)
assert X == F + 1


# ---------------------------------------------------------------------------------------------------------------------------
# the definitions (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------
def unit_targets(table) -> np.ndarray:
    """The unit class rows (K, 16) f32 of a class table, as `set_classes` normalises them (ol_set_classes_kernel)."""
    t = np.array(_host(table), dtype=np.float32)
    if t.ndim != 2 or t.shape[1] != D_E or not 1 <= t.shape[0] <= MAX_CLASSES:
        raise ValueError(f"a class table is (K, 16) float32 with K in 1..{MAX_CLASSES}")
    with np.errstate(all="ignore"):
        return H._unit_rows(t)


def _slot_array(slots, n: int) -> np.ndarray:
    y = _host(slots)
    if y.shape != (n,) or y.dtype.kind not in "iu":
        raise ValueError(f"slots must hold one integer entry per window ({n})")
    return y.astype(np.int64)


def _group_array(groups, n: int, n_groups: int) -> np.ndarray:
    if groups is None:
        return np.zeros(n, dtype=np.int64)
    g = _host(groups)
    if g.shape != (n,) or g.dtype.kind not in "iu":
        raise ValueError(f"groups must hold one integer entry per window ({n})")
    g = g.astype(np.int64)
    if n and g.max() >= n_groups:
        raise ValueError(f"a group index must stay below the number of groups ({n_groups})")
    return np.maximum(g, -1)


def _check_groups(n_groups) -> int:
    if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)) or not 1 <= int(n_groups) <= MAX_GROUPS:
        raise ValueError(f"the number of groups must be an integer in 1..{MAX_GROUPS}")
    return int(n_groups)


def window_weights(slots, n_classes: int, balanced: bool = True, groups=None) -> np.ndarray:
    """w_i (N,) float64.  A window is used when its slot lies in 0..n_classes-1 (and, with `groups`, its group is not
    negative); the others weigh 0.  balanced: 1.0 / (C * n_c) with n_c the used windows of the window's slot and C the slots
    that have any; else 1.0 / N_used.  The weights sum to 1 over the recording (to rounding), whatever groups a plan trains on."""
    y = np.asarray(_host(slots)).astype(np.int64).reshape(-1)
    used = (y >= 0) & (y < int(n_classes))
    if groups is not None:
        used &= np.asarray(_host(groups)).astype(np.int64).reshape(-1) >= 0
    counts = np.bincount(y[used], minlength=int(n_classes)).astype(np.float64)
    per = np.zeros(int(n_classes))
    has = counts > 0
    if has.any():
        per[has] = np.float64(1.0) / (np.float64(has.sum()) * counts[has]) if balanced else np.float64(1.0) / counts.sum()
    w = np.zeros(y.shape[0])
    w[used] = per[y[used]]
    return w


def _u_array(u) -> np.ndarray:
    """the tail inputs as float64 (N, 512); a torch tensor in bf16 or f32 is widened exactly"""
    if hasattr(u, "detach"):
        u = u.detach().float().cpu().numpy()
    a = np.asarray(u)
    if a.ndim != 2 or a.shape[1] != F:
        raise ValueError("u must be (N, 512)")
    a32 = a.astype(np.float32)
    if not np.array_equal(a32.astype(a.dtype), a, equal_nan=True):
        raise ValueError("u must hold float32 (or bfloat16) values")
    return a32.astype(np.float64)


def moments_reference(u, slots, weights, targets, groups=None, n_groups: int = 1):
    """The definition of the moments (module docstring): (G (R, 513, 513) f64, C (R, 513, 16) f64).  u (N, 512); slots (N,);
    weights (N,) f64; targets (K, 16) f32 unit rows, taken as they are; groups (N,) or None (one group).  Host only (numpy)."""
    u64 = _u_array(u)
    n = int(u64.shape[0])
    r_n = _check_groups(n_groups)
    y = _slot_array(slots, n)
    g = _group_array(groups, n, r_n)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    t = np.array(_host(targets), dtype=np.float32)
    if w.shape[0] != n or t.ndim != 2 or t.shape[1] != D_E or not 1 <= t.shape[0] <= MAX_CLASSES:
        raise ValueError("one weight per window and targets (K, 16)")
    t64 = t.astype(np.float64)
    G, Cm = np.zeros((r_n, X, X)), np.zeros((r_n, X, D_E))
    x = np.ones(X)
    with np.errstate(all="ignore"):
        for i in np.nonzero((y >= 0) & (y < t.shape[0]) & (g >= 0))[0].tolist():       # window order; every += is one rounded add
            x[:F] = u64[i]
            G[g[i]] += w[i] * (x[:, None] * x[None, :])
            Cm[g[i]] += w[i] * (x[:, None] * t64[y[i]][None, :])
    return G, Cm


def _plan_table(plans, n_groups: int):
    """plans: (groups, ridge) pairs, groups an iterable of group indices or an int bit mask -> (masks (P,) uint32, ridges (P,) f64)"""
    plans = list(plans)
    if len(plans) > MAX_PLANS:
        raise ValueError(f"at most {MAX_PLANS} plans, got {len(plans)}")
    masks, ridges = np.zeros(len(plans), dtype=np.uint32), np.zeros(len(plans))
    for t, p in enumerate(plans):
        if not isinstance(p, (tuple, list)) or len(p) != 2:
            raise ValueError(f"plan {t} is not a (training groups, ridge) pair")
        grp, lam = p
        if isinstance(grp, (int, np.integer)) and not isinstance(grp, bool):
            mask = int(grp)
        else:
            mask = 0
            for r in grp:
                if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) < n_groups:
                    raise ValueError(f"plan {t}: a training group must be an integer in 0..{n_groups - 1}")
                mask |= 1 << int(r)
        if not 0 <= mask < 1 << n_groups:
            raise ValueError(f"plan {t}: the mask names a group at or above {n_groups}")
        lam = float(lam)
        if not (np.isfinite(lam) and lam >= 0.0):
            raise ValueError(f"plan {t}: the ridge must be finite and >= 0")
        masks[t], ridges[t] = mask, lam
    return masks, ridges


def cholesky_reference(a: np.ndarray):
    """(L, status): the Cholesky factor of the definition (module docstring), right-looking: column k is finished, then every
    element behind it takes its k-th subtraction, so each element sees k ascending.  status 0, or j + 1 for a failing pivot at
    column j (L is then not defined)."""
    low = np.array(a, dtype=np.float64)
    n = low.shape[0]
    with np.errstate(all="ignore"):
        for k in range(n):
            piv = low[k, k]
            if not (np.isfinite(piv) and piv > 0):
                return np.zeros_like(low), k + 1
            low[k, k] = np.sqrt(piv)
            low[k + 1:, k] = low[k + 1:, k] / low[k, k]
            col = low[k + 1:, k]
            low[k + 1:, k + 1:] = low[k + 1:, k + 1:] - col[:, None] * col[None, :]      # (only the lower triangle is read on)
    return np.tril(low), 0


def solve_reference(G, Cm, plans, return_x: bool = False):
    """The definition of plans, Cholesky and solve (module docstring): (W (P, 16, 512) f32, b (P, 16) f32, status (P,) int32).
    G (R, 513, 513), Cm (R, 513, 16) f64; plans as `fit_reference` takes them.  return_x=True: also X (P, 513, 16) f64, the
    solution before it is rounded to f32 (zero for a plan that failed).  Host only (numpy)."""
    G, Cm = np.asarray(G, dtype=np.float64), np.asarray(Cm, dtype=np.float64)
    if G.ndim != 3 or G.shape[1:] != (X, X) or Cm.shape != (G.shape[0], X, D_E):
        raise ValueError("G (R, 513, 513) and C (R, 513, 16)")
    r_n = _check_groups(int(G.shape[0]))
    masks, ridges = _plan_table(plans, r_n)
    n_p = int(masks.shape[0])
    W, b, status = np.zeros((n_p, D_E, F), dtype=np.float32), np.zeros((n_p, D_E), dtype=np.float32), np.zeros(n_p, dtype=np.int32)
    xs = np.zeros((n_p, X, D_E))
    pen = np.arange(F)
    with np.errstate(all="ignore"):
        for t in range(n_p):
            a, rhs = np.zeros((X, X)), np.zeros((X, D_E))
            for r in range(r_n):
                if (int(masks[t]) >> r) & 1:
                    a, rhs = a + G[r], rhs + Cm[r]
            a[pen, pen] = a[pen, pen] + ridges[t]
            low, status[t] = cholesky_reference(a)
            if status[t]:
                continue
            y = rhs.copy()
            for k in range(X):
                y[k] = y[k] / low[k, k]
                y[k + 1:] = y[k + 1:] - low[k + 1:, k, None] * y[k][None, :]
            x = y.copy()
            for i in range(X - 1, -1, -1):                     # (a cumulative sum is sequential: s - p is s + (-p) exactly)
                terms = low[i + 1:, i, None] * x[i + 1:]
                x[i] = np.cumsum(np.concatenate([x[i][None], -terms]), axis=0)[-1] / low[i, i]
            W[t], b[t], xs[t] = x[:F].T.astype(np.float32), x[F].astype(np.float32), x
    return (W, b, status, xs) if return_x else (W, b, status)


def fit_reference(u, slots, targets, plans=None, ridge=0.1, groups=None, n_groups: int = 1, balanced: bool = True) -> dict:
    """The definition of the fit (module docstring).  u (N, 512) stored tail inputs; slots (N,) class slots, negative: not used;
    targets (K, 16) f32 unit rows (`unit_targets`); groups (N,) in 0..n_groups-1 or negative, None: one group; plans: a list of
    (training groups, ridge) pairs, default all groups for every value of `ridge` (a float or a list).  Returns a dict: W
    (P, 16, 512) f32, b (P, 16) f32, status (P,) int32, X (P, 513, 16) f64 (the solution before rounding), G, C, weights, masks (P,) uint32, ridges (P,) f64.  Host only."""
    r_n = _check_groups(n_groups)
    t = np.array(_host(targets), dtype=np.float32)
    if plans is None:
        plans = [((1 << r_n) - 1, lam) for lam in np.asarray(ridge, dtype=np.float64).reshape(-1).tolist()]
    masks, ridges = _plan_table(plans, r_n)
    w = window_weights(slots, int(t.shape[0]), balanced, groups)
    G, Cm = moments_reference(u, slots, w, t, groups, r_n)
    W, b, status, xs = solve_reference(G, Cm, plans, return_x=True)
    return dict(W=W, b=b, status=status, X=xs, G=G, C=Cm, weights=w, masks=masks, ridges=ridges)


def apply_reference(u, W, b, dtype: str = "f32") -> np.ndarray:
    """The definition of the apply (module docstring): u (n, 512) stored tail inputs, W (16, 512) or (P, 16, 512) f32, b (16,)
    or (P, 16) f32, dtype the decoder's compute dtype ('f32' or 'bf16') -> z^ (n, 16) or (P, n, 16) f32.  Host only (numpy)."""
    if dtype not in ("f32", "bf16"):
        raise ValueError("dtype must be 'f32' or 'bf16'")
    u64 = _u_array(u)
    W32, b32 = np.array(_host(W), dtype=np.float32), np.array(_host(b), dtype=np.float32)
    single = W32.ndim == 2
    W32, b32 = (W32[None], b32[None]) if single else (W32, b32)
    if W32.ndim != 3 or W32.shape[1:] != (D_E, F) or b32.shape != (W32.shape[0], D_E):
        raise ValueError("W (P, 16, 512) and b (P, 16)")
    per = 4 if dtype == "f32" else 32                          # products of one matrix instruction
    out = np.zeros((W32.shape[0], u64.shape[0], D_E), dtype=np.float32)
    with np.errstate(all="ignore"):
        for p in range(W32.shape[0]):
            wt = W32[p].astype(np.float64) if dtype == "f32" else round_bf16(W32[p])
            prod = u64[:, None, :] * wt[None, :, :]                                    # exact: (n, 16, 512)
            red = np.zeros((8,) + prod.shape[:2], dtype=np.float32)
            for wave in range(8):
                for c in (wave, wave + 8):
                    chunk = prod[:, :, 32 * c:32 * c + 32]
                    if per == 4:                               # 16-k groups; instruction e of a group takes k = 4 h + e, h = 0..3,
                        for g in range(2):                     # one fused multiply-add per product in that order
                            for e in range(4):
                                for h in range(4):
                                    red[wave] = (red[wave].astype(np.float64) + chunk[:, :, 16 * g + 4 * h + e]).astype(np.float32)
                    else:                                      # one instruction: four partial sums of 8 products, added in order
                        for h in range(4):
                            red[wave] = (red[wave].astype(np.float64) + chunk[:, :, 8 * h:8 * h + 8].sum(axis=2)).astype(np.float32)
            s = red[0]
            for wave in range(1, 8):
                s = s + red[wave]
            z = s + b32[p][None, :]
            ss = np.zeros(z.shape[0], dtype=np.float32)
            for d in range(D_E):
                ss = ss + z[:, d] * z[:, d]
            out[p] = z / np.sqrt(ss)[:, None]
    return out[0] if single else out


def readout_recording(k: int = 8, reps: int = 4, segment: int = 40, seed: int = 0, noise: float = 0.9, wander: float = 0.3):
    """A synthetic person's tail inputs for tests and measurements; nothing about real subjects.  Returns a dict: u
    (k * reps * segment, 512) f32, slots and rep (one per window, int64), W0 (16, 512) f32 and b0 (16,) f32, a random projection
    standing in for the model's.  Class c has a pattern of 512 standard normal numbers; the odd classes 1 and 3 are near-twins of
    0 and 2 (their pattern plus 0.35 standard normal).  Repetition r has an offset wander * a standard normal vector; a window
    is max(pattern[c] + offset[r] + noise * a standard normal vector, 0).  The cue walks through the classes once per
    repetition, `segment` windows each.  Host only; the same arrays for the same arguments."""
    rng = np.random.default_rng(seed)
    pattern = rng.standard_normal((k, F))
    for c in (1, 3):
        if c < k:
            pattern[c] = pattern[c - 1] + 0.35 * rng.standard_normal(F)
    rows, y, rep = [], [], []
    for r in range(reps):
        offset = wander * rng.standard_normal(F)
        for c in range(k):
            rows.append(np.maximum(pattern[c] + offset + noise * rng.standard_normal((segment, F)), 0.0))
            y += [c] * segment
            rep += [r] * segment
    W0 = (0.05 * rng.standard_normal((D_E, F))).astype(np.float32)
    b0 = (0.1 * rng.standard_normal(D_E)).astype(np.float32)
    return dict(u=np.concatenate(rows).astype(np.float32), slots=np.array(y, dtype=np.int64), rep=np.array(rep, dtype=np.int64),
                W0=W0, b0=b0)


def enrolled_rows_reference(emb, slots, k: int, use) -> np.ndarray:
    """The unit rows `enroll` (mix 1) gives from the windows `use` of unit embeddings emb (n, 16) f32: per slot the float64 sum
    in window order, its unit vector, rounded to f32 and normalised as `set_classes` does; a slot without windows gets a
    constant unit row."""
    e64 = np.asarray(emb, dtype=np.float32).astype(np.float64)
    rows = np.full((k, D_E), 0.25, dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in range(k):
            sel = np.asarray(use) & (np.asarray(slots) == c)
            if sel.any():
                s = np.cumsum(e64[sel], axis=0)[-1]
                s2 = np.float64(0.0)
                for d in range(D_E):
                    s2 = s2 + s[d] * s[d]
                rows[c] = (s / np.sqrt(s2)).astype(np.float32)
        return H._unit_rows(rows)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
def _dtype_code(u) -> int:
    import torch
    if u.dtype == torch.float32:
        return _lib.CP_F32
    if u.dtype == torch.bfloat16:
        return _lib.CP_BF16
    raise ValueError("u must be float32 or bfloat16")


def _device_u(u):
    import torch
    if not isinstance(u, torch.Tensor) or u.dim() != 2 or u.shape[1] != F or u.device.type != "cuda":
        raise ValueError("u must be an (N, 512) float32 or bfloat16 tensor on the GPU")
    _dtype_code(u)
    u = u.contiguous()
    return u.clone() if u.data_ptr() % 16 else u


def _scratch(lib, n: int, n_groups: int, n_plans: int, dev):
    import torch
    return torch.empty(lib.cp_online_readout_scratch_bytes(n, n_groups, n_plans), dtype=torch.uint8, device=dev)


def moments(u, slots, weights, targets, groups=None, n_groups: int = 1):
    """`moments_reference` on the device (cp_online_readout_moments): u (N, 512) f32 or bf16 on the GPU; the other arguments as
    the definition takes them, checked before the first launch.  Returns (G (R, 513, 513), C (R, 513, 16)) f64 on the GPU."""
    import torch
    u = _device_u(u)
    n, dev = int(u.shape[0]), u.device
    r_n = _check_groups(n_groups)
    y = _slot_array(slots, n)
    g = _group_array(groups, n, r_n)
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    t = np.ascontiguousarray(np.array(_host(targets), dtype=np.float32))
    if w.shape[0] != n or t.ndim != 2 or t.shape[1] != D_E or not 1 <= t.shape[0] <= MAX_CLASSES:
        raise ValueError("one weight per window and targets (K, 16)")
    lib = _lib.load()
    with torch.cuda.device(dev):
        y_d = torch.from_numpy(np.clip(y, -1, MAX_CLASSES).astype(np.int32)).to(dev)
        g_d = torch.from_numpy(g.astype(np.int32)).to(dev)
        w_d, t_d = torch.from_numpy(w).to(dev), torch.from_numpy(t).to(dev)
        G = torch.empty(r_n, X, X, dtype=torch.float64, device=dev)
        Cm = torch.empty(r_n, X, D_E, dtype=torch.float64, device=dev)
        sc = _scratch(lib, n, r_n, 1, dev)
        _lib.check(lib.cp_online_readout_moments(u.data_ptr() if n else None, _dtype_code(u), n, y_d.data_ptr() if n else None,
                                                 g_d.data_ptr() if n else None, w_d.data_ptr() if n else None, t_d.data_ptr(),
                                                 int(t.shape[0]), r_n, G.data_ptr(), Cm.data_ptr(), sc.data_ptr(), sc.numel(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "cp_online_readout_moments")
    return G, Cm


def solve(G, Cm, plans):
    """`solve_reference` on the device (cp_online_readout_solve, one workgroup per plan): G (R, 513, 513), C (R, 513, 16) f64 on
    the GPU.  Returns (W (P, 16, 512) f32, b (P, 16) f32, status (P,) int32) on the GPU."""
    import torch
    if not isinstance(G, torch.Tensor) or G.dtype != torch.float64 or G.dim() != 3 or tuple(G.shape[1:]) != (X, X) \
            or not isinstance(Cm, torch.Tensor) or Cm.dtype != torch.float64 or tuple(Cm.shape) != (G.shape[0], X, D_E) \
            or G.device.type != "cuda" or Cm.device != G.device:
        raise ValueError("G (R, 513, 513) and C (R, 513, 16) float64 on the GPU")
    r_n = _check_groups(int(G.shape[0]))
    masks, ridges = _plan_table(plans, r_n)
    n_p, dev = int(masks.shape[0]), G.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        G, Cm = G.contiguous(), Cm.contiguous()
        W = torch.zeros(n_p, D_E, F, dtype=torch.float32, device=dev)
        b = torch.zeros(n_p, D_E, dtype=torch.float32, device=dev)
        status = torch.zeros(n_p, dtype=torch.int32, device=dev)
        if n_p:
            sc = _scratch(lib, 1, r_n, n_p, dev)
            _lib.check(lib.cp_online_readout_solve(G.data_ptr(), Cm.data_ptr(), r_n, (C.c_uint32 * n_p)(*masks.tolist()),
                                                   (C.c_double * n_p)(*ridges.tolist()), n_p, W.data_ptr(), b.data_ptr(),
                                                   status.data_ptr(), sc.data_ptr(), sc.numel(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "cp_online_readout_solve")
    return W, b, status


def apply(u, W, b):
    """z^ (P, n, 16) f32 on the GPU of u (n, 512) f32 or bf16 on the GPU under W (P, 16, 512), b (P, 16) f32
    (cp_online_readout_apply): per projection what a push of u's decoder with `set_projection(W[p], b[p])` emits as embeddings,
    bit for bit."""
    import torch
    u = _device_u(u)
    n, dev = int(u.shape[0]), u.device
    W = torch.as_tensor(W, dtype=torch.float32).to(dev).contiguous()
    b = torch.as_tensor(b, dtype=torch.float32).to(dev).contiguous()
    if W.dim() != 3 or tuple(W.shape[1:]) != (D_E, F) or tuple(b.shape) != (W.shape[0], D_E) or W.shape[0] > MAX_PLANS:
        raise ValueError(f"W (P, 16, 512) and b (P, 16), P <= {MAX_PLANS}")
    n_p = int(W.shape[0])
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.empty(n_p, n, D_E, dtype=torch.float32, device=dev)
        if n and n_p:
            sc = _scratch(lib, n, 1, n_p, dev)
            _lib.check(lib.cp_online_readout_apply(u.data_ptr(), _dtype_code(u), n, W.data_ptr(), b.data_ptr(), n_p, out.data_ptr(),
                                                   sc.data_ptr(), sc.numel(), torch.cuda.current_stream(dev).cuda_stream),
                       "cp_online_readout_apply")
    return out


class Readout:
    """What a fit found: W (P, 16, 512) and b (P, 16) f32 on the GPU, status (P,) int32 numpy (0, or j + 1 for a pivot that
    failed at column j: W and b of that plan are zero and it is never installed), plans, the list of (training groups as a
    sorted tuple, ridge) the projections belong to, counts {class id: labelled windows}, ids (K,) int64, and dtype, the compute
    dtype of the decoder whose tail inputs were fitted."""

    def __init__(self, W, b, status, plans, counts, ids, dtype: str):
        self.W, self.b = W, b
        self.status = np.asarray(status, dtype=np.int32).reshape(-1)
        self.plans, self.counts, self.ids, self.dtype = list(plans), dict(counts), _ids_array(ids), dtype

    def _index(self, index) -> int:
        n = int(self.status.shape[0])
        if isinstance(index, bool) or not isinstance(index, (int, np.integer)) or not 0 <= int(index) < n:
            raise IndexError(f"index must be an int in 0..{n - 1}, got {index!r}")
        if self.status[int(index)] != 0:
            raise ValueError(f"plan {int(index)} (ridge {self.plans[int(index)][1]!r}) has no projection: its matrix is not positive "
                             f"definite (pivot {int(self.status[int(index)]) - 1}); raise the ridge")
        return int(index)

    def install(self, decoder, index: int = 0, stream: Optional[int] = None):
        """`decoder.set_projection(W[index], b[index])` on an `OnlineDecoder` (folded or adaptive): `refresh()` keeps it,
        `reset_projection()` drops it.  On a multi-stream decoder built with `stream_projections=True`, `stream=` names the
        stream whose slot takes it (`decoder.set_projection(stream, W[index], b[index])`); without that option the streams
        share one projection and the decoder is refused, as is one with the option but no stream=.
        A plan whose status is not 0 is a ValueError.  Enrol again afterwards (`enroll_reset()`, `enroll`): class rows belong
        to the space they were made in, and the fitted space only approximates the rows it was regressed onto -- at a large
        ridge it shrinks towards the bias and the old rows fit it badly."""
        multi = isinstance(getattr(decoder, "class_ids", None), (list, tuple))
        if multi and stream is not None and getattr(decoder, "stream_projections", False):
            s = decoder._index(stream)
            i = self._index(index)
            decoder.set_projection(s, self.W[i], self.b[i])
            return
        if multi or not hasattr(decoder, "set_projection"):
            raise _lib.CpNativeError("the streams of a multi-stream decoder share one projection: a user's projection cannot be "
                                     "installed for one of them (fit on a stream, install on that user's OnlineDecoder)")
        if stream is not None:
            raise ValueError("stream= goes with a multi-stream decoder")
        i = self._index(index)
        decoder.set_projection(self.W[i], self.b[i])

    def apply(self, u_or_decoder, raw=None, stream: Optional[int] = None):
        """z^ (P, n, 16) f32 on the GPU: every projection applied to u (n, 512) tail inputs on the GPU, or to every window of
        the recording raw (n, 12) through `decoder` (a multi-stream one with `stream`): `Readout.apply(decoder, raw)`.  A plan
        whose status is not 0 gives rows that are not finite."""
        if raw is None:
            return apply(u_or_decoder, self.W, self.b)
        dec = u_or_decoder
        key = dec._index(stream) if isinstance(dec.class_ids, (list, tuple)) else None
        from .online import windows_before
        u = dec._recording_tail_inputs(key, raw, np.arange(windows_before(int(raw.shape[0]), dec.phase)))
        return apply(u, self.W, self.b)


def _decoder_key(decoder, stream):
    multi = isinstance(decoder.class_ids, (list, tuple))
    if multi and stream is None:
        raise ValueError("stream= names the stream of a multi-stream decoder")
    return multi, (decoder._index(stream) if multi else None)


def _default_plans(ridge, plans, n_rep: int):
    if plans is not None:
        return list(plans)
    lam = np.asarray(ridge, dtype=np.float64).reshape(-1)
    return [(tuple(range(n_rep)), float(l)) for l in lam.tolist()]


def _fit_windows(decoder, key, raw, wl, rep, n_rep, plans, balanced, min_windows):
    """the fit on window labels wl (M,) (negative: not labelled) -> (Readout, u of the labelled windows, keep, slots)"""
    import torch
    ids, table, calibrated = decoder._enroll_view(key)
    if ids is None:
        raise _lib.CpNativeError("fit_projection() needs a class table: set_classes() first (its unit rows are the targets)")
    if not calibrated:
        raise _lib.CpNativeError("an AdaBN model has no BatchNorm statistics: calibrate() first, then fit_projection()")
    if isinstance(min_windows, bool) or int(min_windows) < 1:
        raise ValueError("min_windows must be at least 1")
    r_n = _check_groups(n_rep)
    masks, ridges = _plan_table(plans, r_n)
    if masks.shape[0] < 1:
        raise ValueError("at least one plan")
    from .online import _EnrollMixin
    keep, slots, counts = _EnrollMixin._labelled_slots(wl, ids, min_windows)
    groups = None if rep is None else _group_array(np.asarray(_host(rep))[keep], int(keep.size), r_n)
    w = window_weights(slots, int(ids.size), bool(balanced), groups)
    # ---- everything is checked: from here on work is enqueued
    u = decoder._recording_tail_inputs(key, raw, keep)
    targets = unit_targets(table)
    with torch.cuda.device(decoder.device):
        G, Cm = moments(u, slots, w, targets, groups, r_n)
        W, b, status = solve(G, Cm, list(zip(masks.tolist(), ridges.tolist())))
        st = status.cpu().numpy()
    named = [(tuple(r for r in range(r_n) if (int(m) >> r) & 1), float(l)) for m, l in zip(masks.tolist(), ridges.tolist())]
    fit = Readout(W, b, st, named, {int(i): int(c) for i, c in zip(ids, counts)}, ids, decoder.dtype)
    return fit, u, keep, slots


def fit_projection(decoder, raw, labels, *, ridge=0.1, rep=None, plans=None, balanced: bool = True, min_windows: int = 25,
                   stream: Optional[int] = None) -> Readout:
    """A user's projection in closed form (module docstring).  decoder: any of the four online decoders (a multi-stream one
    with `stream`) with a class table; raw (n, 12) f32 on the GPU and labels (n,) per raw sample as `finetune` takes them (a
    stream of its own, read through the electrode map; a label that is not in `class_ids` is a ValueError, as is a class with
    1..min_windows-1 windows).  ridge: a float or a list; rep: (rep (M,), R) as `holdout.repetitions` gives it, one entry per
    window of the recording, default one group; plans: a list of (training repetitions, ridge), default all repetitions for
    every ridge.  The targets are the unit rows of the decoder's current `class_table()`; the tail inputs come from the
    decoder's own encoder (the adaptive form with its statistics frozen).  The decoder is not changed.  One host
    synchronisation: the copy of `status`."""
    from .online import _check_raw, _sample_labels, window_labels
    _, key = _decoder_key(decoder, stream)
    _check_raw(raw)
    wl = window_labels(_sample_labels(labels, raw.shape[0]), decoder.phase)
    rep_w, n_rep = (None, 1) if rep is None else rep
    if rep_w is not None and np.asarray(_host(rep_w)).shape != wl.shape:
        raise ValueError(f"rep must hold one entry per window of the recording ({wl.shape[0]})")
    return _fit_windows(decoder, key, raw, wl, rep_w, n_rep, _default_plans(ridge, plans, n_rep), balanced, min_windows)[0]


def _pick(n_rep: int, lam: np.ndarray, raw_hit, voted_hit, n_cue, status, base) -> dict:
    """the tables of `pick_ridge` from per-(fold, ridge) integers; base: per fold (raw, voted, cue)"""
    n_t = int(lam.shape[0])
    ok = (np.asarray(status).reshape(n_rep, n_t) == 0).all(axis=0)
    rh = np.where(ok, np.asarray(raw_hit).reshape(n_rep, n_t).sum(axis=0), -1)
    vh = np.where(ok, np.asarray(voted_hit).reshape(n_rep, n_t).sum(axis=0), -1)
    nc = np.asarray(n_cue).reshape(n_rep, n_t).sum(axis=0)
    best = None
    for t in range(n_t):                                       # the most voted hits, the larger ridge among equals
        if ok[t] and (best is None or (vh[t], lam[t]) > (vh[best], lam[best])):
            best = t
    b = np.asarray(base, dtype=np.int64).reshape(n_rep, 3).sum(axis=0)
    return dict(ridges=lam, raw_hit=rh.astype(np.int64), voted_hit=vh.astype(np.int64), n_cue=nc.astype(np.int64),
                baseline=dict(raw_hit=int(b[0]), voted_hit=int(b[1]), n_cue=int(b[2])), best=best,
                ridge=None if best is None else float(lam[best]), n_rep=n_rep)


def _check_ridges(ridges) -> np.ndarray:
    lam = np.asarray(_host(ridges), dtype=np.float64).reshape(-1)
    if lam.shape[0] < 1 or not (np.isfinite(lam) & (lam >= 0)).all():
        raise ValueError("ridges must hold at least one finite value >= 0")
    return lam


def pick_ridge_reference(u, expected, ids, table, prior_emb, ridges=RIDGES, folds: Optional[int] = None, vote: int = H.VOTE,
                         min_windows: int = 25, dtype: str = "f32", balanced: bool = True, z=None) -> dict:
    """`pick_ridge` on the definitions alone (`fit_reference`, `apply_reference`, `holdout.holdout_reference`); also fit, what
    `fit_reference` returned for the folds x ridges plans, plans and rep.  u (M, 512): the tail inputs of every window of the recording; expected (M,) per window; table (K, 16) the class table; prior_emb
    (M, 16) f32 the embeddings under the decoder's current projection (the baseline); z: None, or (P, M, 16) f32 embeddings to score in
    place of `apply_reference`'s (a bf16 decoder's, module docstring).  Host only."""
    cid = _ids_array(ids)
    lam = _check_ridges(ridges)
    rep, n_rep = H.repetitions(expected, folds)
    if n_rep < 2:
        raise ValueError("pick_ridge needs at least two repetitions of a cue")
    m = int(rep.shape[0])
    slots = _expected_slots(expected, m, cid).astype(np.int64)
    targets = unit_targets(table)
    loo = H.leave_one_out(n_rep, 1.0, min_windows)
    plans = [(tuple(r for r in range(n_rep) if r != h), float(l)) for h in range(n_rep) for l in lam.tolist()]
    fit = fit_reference(u, slots, targets, plans, groups=np.where(slots >= 0, rep, -1), n_groups=n_rep, balanced=balanced)
    z = apply_reference(u, fit["W"], fit["b"], dtype) if z is None else np.array(_host(z), dtype=np.float32)
    prior = np.array(_host(table), dtype=np.float32)
    rh, vh, nc, base = [], [], [], []
    for h in range(n_rep):
        o = H.holdout_reference(prior_emb, expected, cid, rep, prior, [loo[h]], vote=vote)
        base.append((int(o["pred_hit"][0]), int(o["voted_hit"][0]), int(o["n_cue"][0])))
        for t in range(lam.shape[0]):
            p = h * lam.shape[0] + t
            zz = z[p] if fit["status"][p] == 0 else prior_emb
            o = H.holdout_reference(zz, expected, cid, rep, prior, [loo[h]], vote=vote)
            rh.append(int(o["pred_hit"][0])), vh.append(int(o["voted_hit"][0])), nc.append(int(o["n_cue"][0]))
    out = _pick(n_rep, lam, rh, vh, nc, fit["status"], base)
    out.update(fit=fit, plans=plans, rep=rep)
    return out


def pick_ridge_inputs(u, baseline, expected, ids, table, ridges=RIDGES, folds: Optional[int] = None, vote: int = H.VOTE,
                      min_windows: int = 25, balanced: bool = True) -> dict:
    """`pick_ridge` behind the encoder: u (M, 512) f32 or bf16 on the GPU, the tail inputs of every window of the recording;
    baseline (M, 16) f32 on the GPU, the embeddings under the current projection; expected (M,) per window; ids the K ascending
    class ids and table (K, 16) their class rows.  Returns what `pick_ridge` returns."""
    import torch
    from .online import _EnrollMixin
    cid = _ids_array(ids)
    lam = _check_ridges(ridges)
    vote = H._check_vote(vote)
    rep, n_rep = H.repetitions(expected, folds)
    if n_rep < 2:
        raise ValueError("pick_ridge needs at least two repetitions of a cue")
    if n_rep > MAX_GROUPS:
        raise ValueError(f"the recording has {n_rep} repetitions, more than {MAX_GROUPS}: fold them with folds=")
    n_t = int(lam.shape[0])
    if n_rep * n_t > MAX_PLANS:
        raise ValueError(f"folds x ridges must stay within {MAX_PLANS} plans")
    u = _device_u(u)
    m, dev = int(rep.shape[0]), u.device
    if int(u.shape[0]) != m:
        raise ValueError("expected must hold one entry per window of the recording")
    slots = _expected_slots(expected, m, cid).astype(np.int64)
    if isinstance(min_windows, bool) or int(min_windows) < 1:
        raise ValueError("min_windows must be at least 1")
    _EnrollMixin._labelled_slots(np.where(slots >= 0, cid[np.maximum(slots, 0)], -1), cid, min_windows)
    emb0 = H._device_embeddings(baseline)
    prior = torch.as_tensor(table).to(device=dev, dtype=torch.float32)
    plans = [(tuple(r for r in range(n_rep) if r != h), float(l)) for h in range(n_rep) for l in lam.tolist()]
    groups = np.where(slots >= 0, rep, -1)
    w = window_weights(slots, int(cid.shape[0]), bool(balanced), groups)
    with torch.cuda.device(dev):
        G, Cm = moments(u, slots, w, unit_targets(prior), groups, n_rep)
        W, b, status = solve(G, Cm, plans)
        z = apply(u, W, b)                                     # (P, M, 16): every window, labelled or not
        counts = np.bincount(slots[slots >= 0], minlength=int(cid.shape[0]))
        fit = Readout(W, b, status.cpu().numpy(), plans, {int(i): int(c) for i, c in zip(cid, counts)}, cid,
                      "f32" if u.dtype == torch.float32 else "bf16")
    loo = H.leave_one_out(n_rep, 1.0, int(min_windows))
    rh, vh, nc, base, units = [], [], [], [], {}
    for h in range(n_rep):
        o = H.score_plans(emb0, expected, cid, rep, prior, [loo[h]], vote=vote)
        base.append((int(o["pred_hit"][0]), int(o["voted_hit"][0]), int(o["n_cue"][0])))
        for t in range(n_t):
            p = h * n_t + t
            o = H.score_plans(z[p] if fit.status[p] == 0 else emb0, expected, cid, rep, prior, [loo[h]], vote=vote)
            rh.append(int(o["pred_hit"][0])), vh.append(int(o["voted_hit"][0])), nc.append(int(o["n_cue"][0]))
            units[p] = o["unit"][0]
    out = _pick(n_rep, lam, rh, vh, nc, fit.status, base)
    out.update(readout=fit, rep=rep, logits=None)
    if out["best"] is not None:                                # window i against the rows of the fold that held it out
        t = out["best"]
        assign = H.assign_folds(rep, loo)
        logits = torch.full((m, int(cid.shape[0])), float("nan"), dtype=torch.float32, device=dev)
        for h in range(n_rep):
            sel = torch.from_numpy(np.nonzero(assign == h)[0]).to(dev)
            if sel.numel():
                logits[sel] = H.holdout_logits(z[h * n_t + t], units[h * n_t + t][None].contiguous(), np.zeros(m, dtype=np.int32))[sel]
        out["logits"] = logits
    return out


def pick_ridge(decoder, raw, expected, ridges=RIDGES, folds: Optional[int] = None, stream: Optional[int] = None,
               min_windows: int = 25, balanced: bool = True) -> dict:
    """Which ridge decodes repetitions it has not seen best?  decoder: any of the four online decoders (a multi-stream one with
    `stream`) with a class table; raw (n, 12) f32 on the GPU; expected (M,) per window (`online.expected_commands`,
    `realign.realign_cues`); ridges: 1 or more values >= 0.  Per fold h of `holdout.repetitions(expected, folds)` and ridge:
    the fit on the other repetitions (all folds and ridges in one `cp_online_readout_solve`), applied to the whole recording,
    scored with `holdout.score_plans` on the plan (train = repetitions != h, held out = h; mix 1, so the class rows are
    enrolled in the fitted space from the training repetitions).  The targets are the unit rows of the decoder's current class
    table.  The baseline is the decoder's current projection through `track.embed_recording`, scored the same way.

    Returns a dict: ridges (T,) f64; raw_hit, voted_hit, n_cue (T,) int64, summed over the held-out repetitions, exact
    integers (-1 hits for a ridge whose matrix failed to factor in some fold); baseline, a dict of the same three; best, the
    index with the most voted hits, the larger ridge among equals (None if none is valid); ridge, its value; n_rep; rep;
    readout, the `Readout` of the folds x ridges plans (fold-major); logits (M, K) f32 on the GPU, every window against the
    rows of the fold that held it out under the picked ridge, in the layout `sweep_gate` / `search_grasp_sets` take (None if
    best is None).  The decoder is left as it was: projection, class table, stream state, vote ring, sample count and
    statistics."""
    multi, key = _decoder_key(decoder, stream)
    ids, table, calibrated = decoder._enroll_view(key)
    if ids is None:
        raise _lib.CpNativeError("pick_ridge needs a class table: set_classes() first (its unit rows are the targets)")
    if not calibrated:
        raise _lib.CpNativeError("an AdaBN model has no BatchNorm statistics: calibrate() first, then pick_ridge()")
    from .online import _check_raw, windows_before
    _check_raw(raw)
    m = windows_before(int(raw.shape[0]), decoder.phase)
    _expected_slots(expected, m, _ids_array(ids))
    _check_ridges(ridges)
    u = decoder._recording_tail_inputs(key, raw, np.arange(m))
    # ---- the baseline: the recording through the decoder's own projection, on a copy of what a push changes
    keep = decoder.ws[:H._state_bytes(decoder, multi)].clone()
    seen = decoder._seen.copy() if multi else decoder.n_seen
    try:
        emb0 = H.embed_recording(decoder, raw, key)
    finally:
        decoder.ws[:keep.numel()].copy_(keep)
        if multi:
            decoder._seen[:] = seen
        else:
            decoder.n_seen = seen
    return pick_ridge_inputs(u, emb0, expected, ids, table, ridges, folds, decoder.vote, min_windows, balanced)
