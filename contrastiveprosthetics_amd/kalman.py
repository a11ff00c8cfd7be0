"""Pose filter: a steady-state Kalman stage behind the joint readout.

`kinematics.JointAngles` turns the ridge readout a into a pose joint by joint, with a ring mean and a rate limit: smoothness is
bought with delay.  This module carries a model instead, learnt from the same cued recording: how the hand's joints move together
between windows (from the glove), how wrong the readout is (from held-out predictions), and a gain that weighs the two.  The gain
is iterated to its steady state once, so a window costs one small matrix-vector product.  The device side is cp_online_kf_*
(include/cpnative.h, csrc/online_kalman.cuh); the functions named *_reference and `FilterReference` are the definitions, in numpy
with every operation rounded on its own (no fused multiply-add, no BLAS, no np.linalg), and the device equals them in every bit,
float64 words included.  Throughout, "a sum" runs with its index ascending from +0.0, each product rounded, then added and rounded.

Model.  D joints, 1 <= D <= 32; the state is x = [theta (D), omega (D)] in f32 around the centre c_d = lo_d + ((float) rest_d /
4096.f) * span_d of a `PoseFit` (`centre`); H = [I 0].

Trajectory samples (`triples_reference`).  theta_k = y_k - c, omega_k = theta_k - theta_{k-1}, s_k = [theta_k, omega_k], e_k =
a_k - y_k, each an f32 subtraction; a is the readout's prediction of window k.  Index k counts for group r when windows k-1, k
and k+1 all have group r >= 0 (a group is a repetition; a window with a negative group is not used).

Moments (`moments_reference`).  Per group, over its counted k in window order, in float64: n, G = sum s_k s_k^T, C = sum s_{k+1}
s_k^T, S = sum s_{k+1} s_{k+1}^T (2D x 2D) and E = sum e_{k+1} e_{k+1}^T (D x D): the product of two f32 values is exact, each
term takes one rounded add.

Design (`design_reference`).  A plan is (groups, lam, rho, kappa, T), T in 1..1024.  n is the sum of the groups' n; each of G, C,
S, E is the sum of the groups' matrices in ascending group order, from +0.0, then divided by n.  tr(X) is the sum of the diagonal.
  lambda = (lam * tr(G)) / 2D; the Cholesky factor L of G + lambda I: element (i, j) takes its subtractions L[i][k] * L[j][k] in
    k = 0..j-1 order, one rounded multiply and one rounded subtract each, then the square root (i = j) or the division by L[j][j];
    a pivot that is not > 0 ends the plan.  L L^T X = C^T: forward substitution, row a subtracts L[a][k] * Y[k] for k ascending and
    divides by L[a][a]; backward substitution, row a subtracts L[k][a] * X[k] for k DESCENDING from 2D-1 to a+1 and divides by
    L[a][a].  A = X^T.
  T1 = A C^T (T1[i][j] = sum_k A[i][k] * C[j][k]), AG = A G, T2 = AG A^T, R = ((S - T1) - T1^T) + T2, w0 = (1e-6 * tr(S)) / 2D,
    W[i][j] = rho * (0.5 * (R[i][j] + R[j][i])) off the diagonal and rho * (0.5 * (R[i][i] + R[i][i]) + w0) on it.
  q0 = (1e-6 * tr(E)) / D; Q[i][j] = kappa * E[i][j] off the diagonal and kappa * (E[i][i] + q0) on it.
  P = W.  T times: AP = A P; P-[i][j] = (sum_k AP[i][k] * A[j][k]) + W[i][j] for i >= j, mirrored; the Cholesky factor of
    P-[:D, :D] + Q as above; Z from the two substitutions on the right-hand side P-[:D, :] (D x 2D), K = Z^T; J = I with J[i][k]
    = I[i][k] - K[i][k] for k < D; JP = J P-; KQ = K Q; P[i][j] = (sum_k JP[i][k] * J[j][k]) + (sum_d KQ[i][d] * K[j][d]) for
    i >= j, mirrored.
  M = J A and K, each rounded to f32 once; delta = max|P_T - P_{T-1}| / max|P_T| (P_0 = W).  status: 0; 1 when n < 2D + 1; 2 when
  a pivot of G + lambda I fails; 3 when a pivot of an innovation matrix fails.  With a status M and K are zero and delta is +inf.

Filter step (`FilterReference`), one per stream, rows in order.  o = a - c.  Before the first row whose o is all finite the stream
is not started and `filtered` is NaN; that row sets x = [o, 0].  Later a row with a non-finite o leaves x as it is; otherwise
x'_i = sum_j M[i][j] * x_j continued by sum_j K[i][j] * o_j in the same accumulator.  filtered_d = x_d + c_d.  From `filtered`,
t, q, the rate limit and angle follow `kinematics.JointReference` with smooth = 1: a NaN gives rest, a row whose class is < 0
gives rest while x still updates.  A zeroed state is a valid start.

Score (`sweep_reference`).  Per plan, over the windows whose group is in the plan's test mask, in window order; the filter
restarts wherever the window before has another group.  Eight float64 sums per (plan, joint): the seven of
`kinematics.score_reference` on `filtered` against y, skipping the rows whose `filtered` is NaN, and the sum of (filtered_k -
filtered_{k-1})^2 over the rows whose predecessor belongs to the same run and was not skipped (a jitter measure).

Nothing here is claimed for real subjects: `kinematics.kinematics_recording` is a synthetic person.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from . import kinematics as KN
from . import readout as R
from .track import _host

F = KN.F
MAX_JOINTS = KN.MAX_JOINTS
MAX_GROUPS = KN.MAX_GROUPS
MAX_PLANS = KN.MAX_PLANS
MAX_ITERS = _lib.CP_ONLINE_KF_MAX_ITERS
ONE = KN.ONE
SUMS = _lib.CP_ONLINE_KF_SUMS
KAPPAS = (0.25, 1.0, 4.0)
_STATE_HEAD = 8                                                # OkfState (csrc/online_kalman.cuh): D, started, 6 unused,
_STATE_WORDS = _STATE_HEAD + 2 * MAX_JOINTS + 6 * MAX_JOINTS + 4 * MAX_JOINTS * MAX_JOINTS + 2 * MAX_JOINTS * MAX_JOINTS + MAX_JOINTS * F


# ---------------------------------------------------------------------------------------------------------------------------
# the definitions (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------
def centre(lo, span, rest) -> np.ndarray:
    """c (D,) f32 = lo + ((float) rest / 4096.f) * span: the resting pose in the glove's units, `JointAngles`' expression."""
    lo32, span32, rest32 = KN._check_limits(lo, span, rest, int(np.asarray(_host(lo)).reshape(-1).shape[0]))
    lvl = rest32.astype(np.float32) / np.float32(ONE)
    scaled = lvl * span32
    return lo32 + scaled


def _centre_array(c, d: int) -> np.ndarray:
    c32 = np.array(_host(c), dtype=np.float32).reshape(-1)
    if c32.shape != (d,) or not np.isfinite(c32).all():
        raise ValueError(f"centre must hold one finite value per joint ({d})")
    return c32


def _pair(a, y):
    a32 = np.ascontiguousarray(np.array(_host(a), dtype=np.float32))
    if a32.ndim != 2 or not 1 <= a32.shape[1] <= MAX_JOINTS:
        raise ValueError(f"a must be (N, D) float32 with D in 1..{MAX_JOINTS}")
    return a32, KN._target_array(y, int(a32.shape[0]))


def _groups(groups, n: int, n_groups: int) -> np.ndarray:
    r_n = R._check_groups(n_groups)
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(_host(groups)).astype(np.int64).reshape(-1)
    if g.shape[0] != n:
        raise ValueError(f"groups must hold one entry per window ({n})")
    return np.where((g >= 0) & (g < r_n), g, -1)


def triples_reference(a, y, groups, n_groups: int, c):
    """The trajectory samples (module docstring): (k (n,) int64 the counted indices ascending, group (n,), s_k (n, 2D) f32,
    s_{k+1} (n, 2D) f32, e_{k+1} (n, D) f32).  Host only (numpy)."""
    a32, t = _pair(a, y)
    n, d = t.shape
    g = _groups(groups, n, n_groups)
    c32 = _centre_array(c, d)
    theta = t - c32[None, :]
    omega = np.zeros_like(theta)
    omega[1:] = theta[1:] - theta[:-1]
    s = np.concatenate([theta, omega], axis=1)
    with np.errstate(all="ignore"):
        e = a32 - t
    k = np.arange(1, max(n - 1, 1))
    k = k[(g[k - 1] == g[k]) & (g[k + 1] == g[k]) & (g[k] >= 0)] if n >= 3 else np.zeros(0, dtype=np.int64)
    return k.astype(np.int64), g[k], s[k], s[k + 1], e[k + 1]


def moments_reference(a, y, groups, n_groups: int, c) -> dict:
    """The definition of the moments (module docstring): a dict n (R,) int64, G, C, S (R, 2D, 2D) f64, E (R, D, D) f64.  Host
    only (numpy)."""
    k, gk, s0, s1, e1 = triples_reference(a, y, groups, n_groups, c)
    r_n, d = int(n_groups), int(e1.shape[1])
    n2 = 2 * d
    out = dict(n=np.zeros(r_n, dtype=np.int64), G=np.zeros((r_n, n2, n2)), C=np.zeros((r_n, n2, n2)), S=np.zeros((r_n, n2, n2)),
               E=np.zeros((r_n, d, d)))
    s0, s1, e1 = s0.astype(np.float64), s1.astype(np.float64), e1.astype(np.float64)
    with np.errstate(all="ignore"):
        for i in range(k.shape[0]):                            # window order; every += is one rounded add of an exact product
            r = int(gk[i])
            out["n"][r] += 1
            out["G"][r] += s0[i][:, None] * s0[i][None, :]
            out["C"][r] += s1[i][:, None] * s0[i][None, :]
            out["S"][r] += s1[i][:, None] * s1[i][None, :]
            out["E"][r] += e1[i][:, None] * e1[i][None, :]
    return out


def _mask_of(groups, r_n: int) -> int:
    if isinstance(groups, (int, np.integer)) and not isinstance(groups, bool):
        m = int(groups)
    else:
        m = 0
        for r in groups:
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) < r_n:
                raise ValueError(f"a plan's groups must be integers in 0..{r_n - 1}")
            m |= 1 << int(r)
    if m < 0 or m >> r_n:
        raise ValueError(f"a plan's mask names a group at or above {r_n}")
    return m


def plan_table(plans, n_groups: int):
    """plans: a list of (groups, lam, rho, kappa, T), groups a bit mask or a sequence of group indices -> (masks (P,) int64, lam,
    rho, kappa (P,) f64, iters (P,) int64), checked."""
    r_n = R._check_groups(n_groups)
    plans = list(plans)
    if len(plans) > MAX_PLANS:
        raise ValueError(f"at most {MAX_PLANS} plans")
    masks, lam, rho, kappa, iters = [], [], [], [], []
    for p in plans:
        if len(p) != 5:
            raise ValueError("a plan is (groups, lam, rho, kappa, T)")
        masks.append(_mask_of(p[0], r_n))
        l, r, k = float(p[1]), float(p[2]), float(p[3])
        if not (np.isfinite(l) and l >= 0):
            raise ValueError("a plan's lam must be finite and >= 0")
        if not (np.isfinite(r) and r > 0):
            raise ValueError("a plan's rho must be finite and > 0")
        if not (np.isfinite(k) and k > 0):
            raise ValueError("a plan's kappa must be finite and > 0")
        if isinstance(p[4], bool) or not isinstance(p[4], (int, np.integer)) or not 1 <= int(p[4]) <= MAX_ITERS:
            raise ValueError(f"a plan's T must be an int in 1..{MAX_ITERS}")
        lam.append(l), rho.append(r), kappa.append(k), iters.append(int(p[4]))
    return (np.array(masks, dtype=np.int64), np.array(lam, dtype=np.float64), np.array(rho, dtype=np.float64),
            np.array(kappa, dtype=np.float64), np.array(iters, dtype=np.int64))


def _mm(X, Y):
    """(.., n, m) x (.., m, q): sum_k X[i][k] * Y[k][j], k ascending from +0.0, each product rounded, then added"""
    acc = np.zeros(X.shape[:-1] + (Y.shape[-1],))
    for k in range(X.shape[-1]):
        acc = acc + X[..., :, k, None] * Y[..., k, None, :]
    return acc


def _mmt(X, Y):
    """X Y^T: sum_k X[i][k] * Y[j][k]"""
    return _mm(X, np.swapaxes(Y, -1, -2))


def _trace(X):
    acc = np.zeros(X.shape[:-2])
    for i in range(X.shape[-1]):
        acc = acc + X[..., i, i]
    return acc


def _add_diag(X, v):
    out = X.copy()
    i = np.arange(X.shape[-1])
    out[..., i, i] = X[..., i, i] + v[..., None]
    return out


def _chol(Mx):
    """the Cholesky factor of a batch (P, n, n) in the definition's order -> (L, ok (P,)): ok is False from the first pivot that
    is not > 0 (what follows it in L is not used)"""
    Mx = Mx.copy()
    n = Mx.shape[-1]
    L = np.zeros_like(Mx)
    ok = np.ones(Mx.shape[:-2], dtype=bool)
    for j in range(n):
        piv = Mx[..., j, j]
        ok &= piv > 0
        ljj = np.sqrt(piv)
        L[..., j, j] = ljj
        col = Mx[..., j + 1:, j] / ljj[..., None]
        L[..., j + 1:, j] = col
        Mx[..., j + 1:, j + 1:] = Mx[..., j + 1:, j + 1:] - col[..., :, None] * col[..., None, :]
    return L, ok


def _solve(L, B):
    """L L^T X = B for a batch: forward with k ascending, backward with k descending"""
    X = B.copy()
    n = L.shape[-1]
    for k in range(n):
        X[..., k, :] = X[..., k, :] / L[..., k, k, None]
        X[..., k + 1:, :] = X[..., k + 1:, :] - L[..., k + 1:, k, None] * X[..., k, None, :]
    for k in range(n - 1, -1, -1):
        X[..., k, :] = X[..., k, :] / L[..., k, k, None]
        X[..., :k, :] = X[..., :k, :] - L[..., k, :k, None] * X[..., k, None, :]
    return X


def _mirror(X):
    low = np.tril(X)
    return low + np.swapaxes(np.tril(X, -1), -1, -2)


def design_reference(mom: dict, plans, return_p: bool = False) -> dict:
    """The definition of the design (module docstring): mom as `moments_reference` returns it, plans a list of (groups, lam, rho,
    kappa, T).  Returns a dict: M (P, 2D, 2D) f32, K (P, 2D, D) f32, delta (P,) f64, status (P,) int32; with return_p=True also
    A, W, Q, P, M64 and K64, the float64 matrices behind them.  Host only (numpy)."""
    G, Cm, S, E = (np.asarray(mom[k], dtype=np.float64) for k in ("G", "C", "S", "E"))
    cnt = np.asarray(mom["n"]).astype(np.int64).reshape(-1)
    r_n, n2, d = int(G.shape[0]), int(G.shape[1]), int(E.shape[1])
    if n2 != 2 * d or not 1 <= d <= MAX_JOINTS or cnt.shape[0] != r_n:
        raise ValueError("mom: n (R,), G, C, S (R, 2D, 2D) and E (R, D, D)")
    masks, lam, rho, kappa, iters = plan_table(plans, r_n)
    n_p = int(masks.shape[0])
    out = dict(M=np.zeros((n_p, n2, n2), dtype=np.float32), K=np.zeros((n_p, n2, d), dtype=np.float32), delta=np.full(n_p, np.inf),
               status=np.zeros(n_p, dtype=np.int32))
    if n_p == 0:
        return out
    member = ((masks[:, None] >> np.arange(r_n)[None, :]) & 1) == 1                    # (P, R)
    n = (member * np.maximum(cnt, 0)[None, :]).sum(axis=1)
    status = np.where(n < n2 + 1, 1, 0).astype(np.int32)
    with np.errstate(all="ignore"):
        nd = n.astype(np.float64)[:, None, None]

        def gsum(X):
            acc = np.zeros((n_p,) + X.shape[1:])
            for r in range(r_n):
                acc = np.where(member[:, r, None, None], acc + X[r][None], acc)
            return acc / nd

        Gs, Cs, Ss, Es = gsum(G), gsum(Cm), gsum(S), gsum(E)
        lamv = (lam * _trace(Gs)) / np.float64(n2)
        L, ok = _chol(_add_diag(Gs, lamv))
        status = np.where((status == 0) & ~ok, 2, status).astype(np.int32)
        A = np.swapaxes(_solve(L, np.swapaxes(Cs, -1, -2)), -1, -2)
        T1 = _mmt(A, Cs)
        T2 = _mmt(_mm(A, Gs), A)
        Rm = ((Ss - T1) - np.swapaxes(T1, -1, -2)) + T2
        w0 = (1e-6 * _trace(Ss)) / np.float64(n2)
        W = rho[:, None, None] * _add_diag(0.5 * (Rm + np.swapaxes(Rm, -1, -2)), w0)
        q0 = (1e-6 * _trace(Es)) / np.float64(d)
        Q = kappa[:, None, None] * _add_diag(Es, q0)
        P, Pprev = W.copy(), W.copy()
        Kt = np.zeros((n_p, n2, d))
        eye = np.broadcast_to(np.eye(n2), (n_p, n2, n2))

        def jmat(Km):
            J = eye.copy()
            J[:, :, :d] = eye[:, :, :d] - Km
            return J

        for it in range(int(iters.max())):
            live = (status == 0) & (it < iters)
            if not live.any():
                break
            Pm = _mirror(_mmt(_mm(A, P), A) + W)
            Ls, ok = _chol(Pm[:, :d, :d] + Q)
            status = np.where(live & ~ok, 3, status).astype(np.int32)
            live = live & ok
            Kn = np.swapaxes(_solve(Ls, Pm[:, :d, :]), -1, -2)
            J = jmat(Kn)
            Pn = _mirror(_mmt(_mm(J, Pm), J) + _mmt(_mm(Kn, Q), Kn))
            sel = live[:, None, None]
            Pprev = np.where(sel, P, Pprev)
            P = np.where(sel, Pn, P)
            Kt = np.where(sel, Kn, Kt)
        Mx = _mm(jmat(Kt), A)
        delta = np.abs(P - Pprev).max(axis=(1, 2)) / np.abs(P).max(axis=(1, 2))
    good = status == 0
    out["M"][good] = Mx[good].astype(np.float32)
    out["K"][good] = Kt[good].astype(np.float32)
    out["delta"][good] = delta[good]
    out["status"] = status
    if return_p:
        out.update(A=A, W=W, Q=Q, P=P, M64=Mx, K64=Kt)
    return out


def _check_model(M, K):
    M32, K32 = np.array(_host(M), dtype=np.float32), np.array(_host(K), dtype=np.float32)
    d = int(K32.shape[-1]) if K32.ndim >= 2 else 0
    if not 1 <= d <= MAX_JOINTS or M32.shape[-2:] != (2 * d, 2 * d) or K32.shape[-2:] != (2 * d, d) or M32.shape[:-2] != K32.shape[:-2]:
        raise ValueError(f"M (.., 2D, 2D) and K (.., 2D, D) with D in 1..{MAX_JOINTS}")
    return M32, K32, d


def filter_step(M, K, x, started: bool, o):
    """One filter step (module docstring) on numpy f32 arrays: M (2D, 2D), K (2D, D), x (2D,), o (D,) -> (x', started')."""
    d = int(o.shape[0])
    if not np.isfinite(o).all():
        return x, started
    if not started:
        return np.concatenate([o, np.zeros(d, dtype=np.float32)]), True
    acc = np.zeros(2 * d, dtype=np.float32)
    for j in range(2 * d):
        acc = acc + M[:, j] * x[j]
    for j in range(d):
        acc = acc + K[:, j] * o[j]
    return acc, True


class FilterReference:
    """The definition of one stream's filter and integer tail (module docstring).  M (2D, 2D), K (2D, D) f32; lo, span (D,) f32
    and rest (D,) integers in 0..4096; rate 1..4096.  `push(a, cls=None)` takes the next rows of the readout a (n, D) f32 and
    optionally their classes (n,) (< 0: none) and returns (filtered (n, D) f32, pose (n, D) int32, angle (n, D) f32); the state
    carries over, so any cut of the rows into calls gives the same rows.  Host only (numpy)."""

    def __init__(self, M, K, lo, span, rest, rate: int = ONE):
        self.M, self.K, self.D = _check_model(M, K)
        if self.M.ndim != 2:
            raise ValueError("M (2D, 2D) and K (2D, D) of one plan")
        self.lo, self.span, self.rest = KN._check_limits(lo, span, rest, self.D)
        self.rate = KN._check_stage(1, rate)[1]
        self.c = centre(self.lo, self.span, self.rest)
        self.events = set()                                    # what has happened so far: not_started, start, hold, none, clamp_low,
        self.reset()                                           # clamp_high, rise_limited, fall_limited (a test aid)

    def reset(self):
        self.x = np.zeros(2 * self.D, dtype=np.float32)
        self.started = False
        self.out = np.zeros(self.D, dtype=np.int64)

    def push(self, a, cls=None):
        a32 = np.array(_host(a), dtype=np.float32)
        if a32.ndim != 2 or a32.shape[1] != self.D:
            raise ValueError(f"a must be (n, {self.D}) float32")
        n = int(a32.shape[0])
        c = None
        if cls is not None:
            c = np.asarray(_host(cls)).astype(np.int64).reshape(-1)
            if c.shape[0] != n:
                raise ValueError(f"cls must hold one entry per row ({n})")
        filt = np.full((n, self.D), np.nan, dtype=np.float32)
        pose, angle = np.zeros((n, self.D), dtype=np.int32), np.zeros((n, self.D), dtype=np.float32)
        one = np.float32(ONE)
        with np.errstate(all="ignore"):
            for i in range(n):
                o = a32[i] - self.c
                was = self.started
                self.x, self.started = filter_step(self.M, self.K, self.x, self.started, o)
                self.events.add("not_started" if not self.started else "start" if not was else "run" if np.isfinite(o).all() else "hold")
                if self.started:
                    filt[i] = self.x[:self.D] + self.c
                t = (filt[i] - self.lo) / self.span
                f = np.minimum(np.maximum(np.where(np.isnan(t), np.float32(0), t), np.float32(0)), np.float32(1))
                q = np.rint(f * one).astype(np.int64)
                q = np.where(np.isnan(t), self.rest, q)
                if c is not None and c[i] < 0:
                    q = self.rest.astype(np.int64)
                for name, hit in (("clamp_low", (t < 0).any()), ("clamp_high", (t > 1).any()), ("none", c is not None and c[i] < 0),
                                  ("rise_limited", (q > self.out + self.rate).any()), ("fall_limited", (q < self.out - self.rate).any())):
                    if hit:
                        self.events.add(name)
                self.out = np.where(q > self.out, np.minimum(self.out + self.rate, q), np.maximum(self.out - self.rate, q))
                pose[i] = self.out
                lvl = self.out.astype(np.float32) / one
                scaled = lvl * self.span
                angle[i] = self.lo + scaled
        return filt, pose, angle

    def state(self) -> dict:
        return dict(started=bool(self.started), x=self.x.copy(), out=self.out.astype(np.int64).copy())


def sweep_reference(a, y, groups, test_masks, M, K, c, return_filtered: bool = False):
    """The definition of the score (module docstring): a, y (N, D) f32, groups (N,), test_masks (P,) bit masks of groups, M
    (P, 2D, 2D), K (P, 2D, D) f32, c (D,) -> sums (P, D, 8) f64 [, filtered (P, N, D) f32, NaN on the rows outside a plan's mask].
    Host only (numpy)."""
    a32, t = _pair(a, y)
    n, d = t.shape
    M32, K32, dm = _check_model(M, K)
    masks = KN._mask_array(test_masks)
    g = np.asarray(_host(groups)).astype(np.int64).reshape(-1)
    if M32.ndim != 3 or dm != d or g.shape[0] != n or masks.shape[0] != M32.shape[0]:
        raise ValueError("one group per row, one test mask per plan, M (P, 2D, 2D) and K (P, 2D, D)")
    c32 = _centre_array(c, d)
    n_p = int(masks.shape[0])
    sums = np.zeros((n_p, d, SUMS))
    filt = np.full((n_p, n, d), np.nan, dtype=np.float32)
    t64 = t.astype(np.float64)
    with np.errstate(all="ignore"):
        for p in range(n_p):
            x, started = np.zeros(2 * d, dtype=np.float32), False
            prev = np.full(d, np.nan)
            for k in range(n):
                if not (0 <= g[k] < MAX_GROUPS and (int(masks[p]) >> int(g[k])) & 1):
                    continue
                if k == 0 or g[k - 1] != g[k]:
                    x, started = np.zeros(2 * d, dtype=np.float32), False
                    prev = np.full(d, np.nan)
                x, started = filter_step(M32[p], K32[p], x, started, a32[k] - c32)
                if started:
                    filt[p, k] = x[:d] + c32
                q, yy = filt[p, k].astype(np.float64), t64[k]
                has = ~np.isnan(q)
                e = q - yy
                dq = q - prev
                terms = (np.ones(d), yy, yy * yy, q, q * q, yy * q, e * e)
                for j, v in enumerate(terms):
                    sums[p, :, j] = np.where(has, sums[p, :, j] + v, sums[p, :, j])
                sums[p, :, 7] = np.where(has & ~np.isnan(prev), sums[p, :, 7] + dq * dq, sums[p, :, 7])
                prev = q
    return (sums, filt) if return_filtered else sums


def unfiltered_sums(a, y, groups, test_masks) -> np.ndarray:
    """The eight sums of `sweep_reference` for the readout a itself (no filter): (P, D, 8) f64.  Host only (numpy)."""
    a32, t = _pair(a, y)
    n, d = t.shape
    masks = KN._mask_array(test_masks)
    g = np.asarray(_host(groups)).astype(np.int64).reshape(-1)
    sums = np.zeros((masks.shape[0], d, SUMS))
    sums[:, :, :7] = KN.score_reference(np.broadcast_to(a32, (masks.shape[0], n, d)), t, g, masks)
    a64 = a32.astype(np.float64)
    with np.errstate(all="ignore"):
        for p in range(masks.shape[0]):
            prev = np.full(d, np.nan)
            for k in range(n):
                if not (0 <= g[k] < MAX_GROUPS and (int(masks[p]) >> int(g[k])) & 1):
                    continue
                if k == 0 or g[k - 1] != g[k]:
                    prev = np.full(d, np.nan)
                q = a64[k]
                dq = q - prev
                sums[p, :, 7] = np.where(~np.isnan(q) & ~np.isnan(prev), sums[p, :, 7] + dq * dq, sums[p, :, 7])
                prev = q
    return sums


def _pick_grid(kappas, rhos, lam, iters, n_rep: int):
    kap = np.asarray(list(kappas), dtype=np.float64).reshape(-1)
    rho = np.asarray(list(rhos), dtype=np.float64).reshape(-1)
    if kap.shape[0] < 1 or rho.shape[0] < 1:
        raise ValueError("kappas and rhos must hold at least one value")
    if n_rep < 2:
        raise ValueError("pick_filter needs at least two repetitions")
    if n_rep * kap.shape[0] * rho.shape[0] > MAX_PLANS:
        raise ValueError(f"folds x rhos x kappas must stay within {MAX_PLANS} plans")
    rows = [(float(r), float(k)) for r in rho.tolist() for k in kap.tolist()]
    plans = [(tuple(g for g in range(n_rep) if g != h), float(lam), r, k, iters) for h in range(n_rep) for r, k in rows]
    plan_table(plans, n_rep)
    tests = np.array([1 << h for h in range(n_rep) for _ in rows], dtype=np.int64)
    return rows, plans, tests


def _pick_tables(fold_sums, status, delta, bare_folds, rows, n_rep: int) -> dict:
    """the tables of `pick_filter` from fold_sums (R, rows, D, 8), status and delta (R, rows) and bare_folds (R, D, 8)"""
    n_rows = len(rows)
    total = np.zeros((1 + n_rows,) + fold_sums.shape[2:])
    for h in range(n_rep):                                     # fold order, one rounded add each
        total[0] = total[0] + bare_folds[h]
        total[1:] = total[1:] + fold_sums[h]
    ok = np.concatenate([[True], (np.asarray(status).reshape(n_rep, n_rows) == 0).all(axis=0)])
    met = KN.metrics(total[..., :7])
    with np.errstate(all="ignore"):
        pairs = np.maximum(total[..., 0] - 1.0, 1.0)
        jitter = np.sqrt(total[..., 7] / pairs).mean(axis=-1)
    table = np.full((1 + n_rows, 4), np.nan)
    table[1:, 0] = [r for r, _ in rows]
    table[1:, 1] = [k for _, k in rows]
    table[:, 2] = met["rmse_mean"]
    table[:, 3] = jitter
    pick = None
    for i in range(1 + n_rows):                                # the smallest RMSE; among equals the unfiltered row, then the larger kappa
        v = table[i, 2]
        if not ok[i] or not np.isfinite(v):
            continue
        key = (v, 0 if i == 0 else 1, -table[i, 1] if i else 0.0)
        if pick is None or key < pick[0]:
            pick = (key, i)
    pick = None if pick is None else pick[1]
    filt = [i for i in range(1, 1 + n_rows) if ok[i] and np.isfinite(table[i, 2])]
    best_f = min(filt, key=lambda i: (table[i, 2], -table[i, 1])) if filt else None
    return dict(table=table, rows=[None] + list(rows), sums=total, fold_sums=fold_sums, bare_fold_sums=bare_folds, ok=ok,
                delta=np.asarray(delta).reshape(n_rep, n_rows), pick=pick, best_filter=best_f, n_rep=n_rep,
                rho=None if not pick else float(table[pick, 0]), kappa=None if not pick else float(table[pick, 1]),
                rmse=met["rmse"], rmse_mean=met["rmse_mean"], jitter=jitter)


def pick_filter_reference(a, y, rep, fit, kappas=KAPPAS, rhos=(1.0,), lam: float = 1e-3, iters: int = 128) -> dict:
    """`pick_filter` on the definitions alone.  Host only (numpy)."""
    a32, t = _pair(a, y)
    groups, n_rep = KN._rep_groups(rep, int(t.shape[0]))
    rows, plans, tests = _pick_grid(kappas, rhos, lam, iters, n_rep)
    c = centre(fit.lo, fit.span, fit.rest)
    des = design_reference(moments_reference(a32, t, groups, n_rep, c), plans)
    sums = sweep_reference(a32, t, groups, tests, des["M"], des["K"], c)
    bare = unfiltered_sums(a32, t, groups, [1 << h for h in range(n_rep)])
    return _pick_tables(sums.reshape(n_rep, len(rows), t.shape[1], SUMS), des["status"].reshape(n_rep, len(rows)),
                        des["delta"].reshape(n_rep, len(rows)), bare, rows, n_rep)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
def _device_a(a, y):
    """a (N, D) f32 on the GPU (a numpy array is uploaded to the current device) and the checked targets"""
    import torch
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(np.array(_host(a), dtype=np.float32))).cuda()
    if a.dtype != torch.float32 or a.dim() != 2 or a.device.type != "cuda" or not 1 <= a.shape[1] <= MAX_JOINTS:
        raise ValueError(f"a must be (N, D) float32 on the GPU with D in 1..{MAX_JOINTS}")
    a = a.contiguous()
    return a, KN._target_array(y, int(a.shape[0]))


def _fptr(v: np.ndarray):
    return v.ctypes.data_as(C.POINTER(C.c_float))


def moments(a, y, groups, n_groups: int, c) -> dict:
    """`moments_reference` on the device (cp_online_kf_moments): a (N, D) f32 on the GPU (or numpy), y (N, D) f32.  Returns a
    dict of tensors on the GPU: n (R,) int32, G, C, S (R, 2D, 2D) f64, E (R, D, D) f64."""
    import torch
    a, t = _device_a(a, y)
    n, d = t.shape
    g = _groups(groups, n, n_groups)
    c32 = _centre_array(c, d)
    r_n, dev = int(n_groups), a.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        y_d, g_d = torch.from_numpy(t).to(dev), torch.from_numpy(g.astype(np.int32)).to(dev)
        out = dict(n=torch.empty(r_n, dtype=torch.int32, device=dev), E=torch.empty(r_n, d, d, dtype=torch.float64, device=dev))
        for k in ("G", "C", "S"):
            out[k] = torch.empty(r_n, 2 * d, 2 * d, dtype=torch.float64, device=dev)
        _lib.check(lib.cp_online_kf_moments(a.data_ptr() if n else None, y_d.data_ptr() if n else None, g_d.data_ptr() if n else None,
                                            n, d, r_n, _fptr(c32), out["G"].data_ptr(), out["C"].data_ptr(), out["S"].data_ptr(),
                                            out["E"].data_ptr(), out["n"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "cp_online_kf_moments")
    return out


def design(mom: dict, plans) -> dict:
    """`design_reference` on the device (cp_online_kf_design): mom as `moments` returns it.  Returns a dict of tensors on the GPU:
    M (P, 2D, 2D) f32, K (P, 2D, D) f32, delta (P,) f64, status (P,) int32; nothing visits the host."""
    import torch
    G, E = mom["G"], mom["E"]
    if not all(isinstance(mom[k], torch.Tensor) and mom[k].device.type == "cuda" for k in ("n", "G", "C", "S", "E")):
        raise ValueError("mom must hold the tensors `moments` returns")
    r_n, n2, d = int(G.shape[0]), int(G.shape[1]), int(E.shape[1])
    if n2 != 2 * d or tuple(mom["C"].shape) != (r_n, n2, n2) or tuple(mom["S"].shape) != (r_n, n2, n2) or tuple(E.shape) != (r_n, d, d):
        raise ValueError("mom: n (R,), G, C, S (R, 2D, 2D) and E (R, D, D)")
    masks, lam, rho, kappa, iters = plan_table(plans, r_n)
    n_p, dev = int(masks.shape[0]), G.device
    lib = _lib.load()
    table = (_lib.cp_online_kf_plan * max(n_p, 1))()
    for i in range(n_p):
        table[i].groups, table[i].iters = int(masks[i]), int(iters[i])
        table[i].lam, table[i].rho, table[i].kappa = float(lam[i]), float(rho[i]), float(kappa[i])
    with torch.cuda.device(dev):
        out = dict(M=torch.empty(n_p, n2, n2, dtype=torch.float32, device=dev), K=torch.empty(n_p, n2, d, dtype=torch.float32, device=dev),
                   delta=torch.empty(n_p, dtype=torch.float64, device=dev), status=torch.empty(n_p, dtype=torch.int32, device=dev))
        if n_p:
            sc = torch.empty(lib.cp_online_kf_design_bytes(n_p), dtype=torch.uint8, device=dev)
            _lib.check(lib.cp_online_kf_design(*(mom[k].contiguous().data_ptr() for k in ("G", "C", "S", "E", "n")), d, r_n, table, n_p,
                                               out["M"].data_ptr(), out["K"].data_ptr(), out["delta"].data_ptr(), out["status"].data_ptr(),
                                               sc.data_ptr(), sc.numel(), torch.cuda.current_stream(dev).cuda_stream),
                       "cp_online_kf_design")
    return out


def sweep(a, y, groups, test_masks, M, K, c, return_filtered: bool = False):
    """`sweep_reference` on the device (cp_online_kf_sweep): M (P, 2D, 2D) and K (P, 2D, D) f32 on the GPU as `design` returns
    them.  Returns sums (P, D, 8) f64 on the GPU [, filtered (P, N, D) f32]."""
    import torch
    a, t = _device_a(a, y)
    n, d = t.shape
    dev = a.device
    masks = KN._mask_array(test_masks)
    g = np.asarray(_host(groups)).astype(np.int64).reshape(-1)
    M = torch.as_tensor(M, dtype=torch.float32).to(dev).contiguous()
    K = torch.as_tensor(K, dtype=torch.float32).to(dev).contiguous()
    n_p = int(masks.shape[0])
    if g.shape[0] != n or tuple(M.shape) != (n_p, 2 * d, 2 * d) or tuple(K.shape) != (n_p, 2 * d, d):
        raise ValueError("one group per row, one test mask per plan, M (P, 2D, 2D) and K (P, 2D, D)")
    c32 = _centre_array(c, d)
    lib = _lib.load()
    with torch.cuda.device(dev):
        y_d = torch.from_numpy(t).to(dev)
        g_d = torch.from_numpy(np.clip(g, -1, MAX_GROUPS).astype(np.int32)).to(dev)
        sums = torch.zeros(n_p, d, SUMS, dtype=torch.float64, device=dev)
        filt = torch.empty(n_p, n, d, dtype=torch.float32, device=dev) if return_filtered else None
        if n_p:
            _lib.check(lib.cp_online_kf_sweep(a.data_ptr() if n else None, y_d.data_ptr() if n else None, g_d.data_ptr() if n else None, n, d,
                                              (C.c_uint32 * n_p)(*masks.tolist()), n_p, M.data_ptr(), K.data_ptr(), _fptr(c32),
                                              sums.data_ptr(), None if filt is None or not n else filt.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream), "cp_online_kf_sweep")
    return (sums, filt) if return_filtered else sums


def _crossfit_plans(rep, n: int):
    if rep is None:
        raise ValueError("a cross-fit needs the repetition of every window")
    groups, n_rep = KN._rep_groups(rep, n)
    if n_rep < 2:
        raise ValueError("a cross-fit needs at least two repetitions")
    return groups, n_rep, [tuple(r for r in range(n_rep) if r != h) for h in range(n_rep)]


def crossfit_reference(u, y, rep, ridge: float = 0.01) -> np.ndarray:
    """`crossfit_inputs` on the definitions (`kinematics.fit_reference`, `pose_reference`).  Host only (numpy)."""
    u32 = np.asarray(_host(u), dtype=np.float32)
    t = KN._target_array(y, int(u32.shape[0]))
    groups, n_rep, folds = _crossfit_plans(rep, int(t.shape[0]))
    fit = KN.fit_reference(u32, t, [(f, float(ridge)) for f in folds], groups=groups, n_groups=n_rep)
    if (fit["status"] != 0).any():
        raise ValueError("a fold's readout has no solution: raise the ridge")
    a = np.full(t.shape, np.nan, dtype=np.float32)
    for h in range(n_rep):
        a[groups == h] = KN.pose_reference(u32[groups == h], fit["W"][h], fit["b"][h])
    return a


def crossfit_inputs(u, y, rep, ridge: float = 0.01):
    """`crossfit_pose` behind the encoder: u (N, 512) f32 or bf16 on the GPU, the tail inputs of the windows with a target, and
    y (N, D) f32 their targets.  Per fold the readout on the other repetitions (`kinematics.moments`, `solve`), then the shipped
    device apply; row k is the prediction of the plan that did not see window k's repetition, NaN where it has none."""
    import torch
    u = R._device_u(u)
    t = KN._target_array(y, int(u.shape[0]))
    groups, n_rep, folds = _crossfit_plans(rep, int(t.shape[0]))
    dev = u.device
    with torch.cuda.device(dev):
        G, Cm = KN.moments(u, t, None, groups, n_rep)
        W, b, status = KN.solve(G, Cm, [(f, float(ridge)) for f in folds], int(t.shape[1]))
        if status.cpu().numpy().any():
            raise ValueError("a fold's readout has no solution: raise the ridge")
        pred = KN.apply(u, W, b)                               # (R, N, D)
        idx = torch.from_numpy(np.clip(groups, 0, n_rep - 1)).to(dev)
        a = pred[idx, torch.arange(int(t.shape[0]), device=dev)]
        a = torch.where(torch.from_numpy(groups >= 0).to(dev)[:, None], a, torch.full_like(a, float("nan")))
    return a.contiguous()


def crossfit_pose(decoder, raw, glove, rep, ridge: float = 0.01, lag: int = 0, stream: Optional[int] = None):
    """a (N, D) f32 on the GPU: every window of the recording predicted by the readout plan that did not see its repetition
    (`fit_pose`'s moments and solve on leave-a-repetition-out plans at one ridge, then the shipped device apply); N is the number
    of windows with a target at this lag.  The rows of windows without a repetition (rep < 0) are NaN.  decoder, raw and glove as
    `fit_pose` takes them; rep: (rep (M,), R) per window (`holdout.repetitions`).  The decoder is left as it was."""
    key, g, m = KN._recording(decoder, raw, glove, stream, "crossfit_pose")
    y = KN.window_targets(g, decoder.phase, lag)
    n = int(y.shape[0])
    if n < 1:
        raise ValueError("the recording has no window with a target")
    if rep is None:
        raise ValueError("a cross-fit needs the repetition of every window")
    groups, n_rep = KN._rep_groups(rep, m)
    u = decoder._recording_tail_inputs(key, raw, np.arange(n))
    return crossfit_inputs(u, y, (groups[:n], n_rep), ridge)


class FilterFit:
    """What `fit_filter` found: M (P, 2D, 2D) and K (P, 2D, D) f32 on the GPU, delta (P,) f64 and status (P,) int32 numpy (0, or
    1: too few samples, 2 / 3: a matrix is not positive definite; M and K of that plan are zero and it is never installed), plans,
    the list of (groups as a sorted tuple, lam, rho, kappa, T), counts {group: samples}, centre (D,) f32 and pose, the `PoseFit`
    whose readout the filter stands behind."""

    def __init__(self, M, K, delta, status, plans, counts, centre_, pose):
        self.M, self.K = M, K
        self.delta = np.asarray(delta, dtype=np.float64).reshape(-1)
        self.status = np.asarray(status, dtype=np.int32).reshape(-1)
        self.plans, self.counts = list(plans), dict(counts)
        self.centre, self.pose = np.asarray(centre_, dtype=np.float32), pose
        self.n_joints = int(K.shape[2])

    def _index(self, index) -> int:
        n = int(self.status.shape[0])
        if isinstance(index, bool) or not isinstance(index, (int, np.integer)) or not 0 <= int(index) < n:
            raise IndexError(f"index must be an int in 0..{n - 1}, got {index!r}")
        if self.status[int(index)] != 0:
            raise ValueError(f"plan {int(index)} has no filter (status {int(self.status[int(index)])}): too few samples, or a matrix "
                             f"is not positive definite")
        return int(index)

    def install(self, stage, index: int = 0, stream: Optional[int] = None):
        """Install plan `index` with the readout it stands behind into a `PoseFilter` stage (`stage.set_model`): on a
        multi-stream source into `stream`.  That stream of the stage restarts.  A plan whose status is not 0 is a ValueError."""
        i = self._index(index)
        p = self.pose
        j = p._index(0)                                        # (the readout `JointAngles` installs from a PoseFit)
        model = (p.W[j], p.b[j], p.lo, p.span, p.rest, self.M[i], self.K[i])
        if stage.multi:
            if stream is None:
                raise ValueError("stream= names the stream of a multi-stream source")
            stage.set_model(stream, *model)
        else:
            if stream is not None:
                raise ValueError("stream= goes with a multi-stream source")
            stage.set_model(*model)


def fit_filter(a, y, rep, fit, lam: float = 1e-3, rho: float = 1.0, kappa: float = 1.0, iters: int = 128, plans=None) -> FilterFit:
    """The filter in closed form (module docstring).  a (N, D) f32 on the GPU, the readout's prediction of every window, best from
    `crossfit_pose` so that its error is a held-out error; y (N, D) f32 the targets (`kinematics.window_targets`); rep: (rep (N,),
    R) per window or None (one group); fit: the `PoseFit` whose readout the filter stands behind (its lo, span and rest give the
    centre).  plans: a list of (groups, lam, rho, kappa, T), default one plan on every group with the keyword values.  One host
    synchronisation: the copy of status and delta."""
    import torch
    a, t = _device_a(a, y)
    if int(t.shape[1]) != fit.n_joints:
        raise ValueError("a, y and the pose fit disagree on the number of joints")
    groups, n_rep = KN._rep_groups(rep, int(t.shape[0]))
    if plans is None:
        plans = [((1 << n_rep) - 1, lam, rho, kappa, iters)]
    masks, lams, rhos, kappas, its = plan_table(plans, n_rep)
    if masks.shape[0] < 1:
        raise ValueError("at least one plan")
    c = centre(fit.lo, fit.span, fit.rest)
    with torch.cuda.device(a.device):
        mom = moments(a, t, groups, n_rep, c)
        des = design(mom, plans)
        st, delta, cnt = des["status"].cpu().numpy(), des["delta"].cpu().numpy(), mom["n"].cpu().numpy()
    named = [(tuple(r for r in range(n_rep) if (int(mk) >> r) & 1), float(l), float(r_), float(k), int(i))
             for mk, l, r_, k, i in zip(masks.tolist(), lams.tolist(), rhos.tolist(), kappas.tolist(), its.tolist())]
    return FilterFit(des["M"], des["K"], delta, st, named, {r: int(cnt[r]) for r in range(n_rep)}, c, fit)


def pick_filter(a, y, rep, fit, kappas=KAPPAS, rhos=(1.0,), lam: float = 1e-3, iters: int = 128) -> dict:
    """Which noise scales track the pose of repetitions the filter has not seen best?  a, y, rep and fit as `fit_filter` takes
    them.  Per fold h and (rho, kappa): the design on the other repetitions, then the device sweep (`sweep`) on repetition h.

    NOTE: a on the TRAINING repetitions of a fold came from readout plans that saw the held-out repetition (`crossfit_pose`
    holds out one repetition at a time, not two).  This nesting is not resolved here; the measurement noise of a fold is therefore
    estimated from predictions that are held out with respect to their own repetition only.

    Returns a dict: table (1 + rows, 4) f64 with columns rho, kappa, mean held-out RMSE over the joints and the jitter (root mean
    squared window-to-window change, mean over the joints); row 0 is the unfiltered readout (rho and kappa NaN); rows, the (rho,
    kappa) of every row; sums (1 + rows, D, 8) f64, the folds added in fold order, fold_sums and bare_fold_sums; ok; delta (R,
    rows); pick, the row with the smallest RMSE, among equals the unfiltered row first, then the larger kappa; best_filter, the
    best filtered row; rho, kappa of the pick (None for row 0)."""
    import torch
    a, t = _device_a(a, y)
    groups, n_rep = KN._rep_groups(rep, int(t.shape[0]))
    rows, plans, tests = _pick_grid(kappas, rhos, lam, iters, n_rep)
    c = centre(fit.lo, fit.span, fit.rest)
    with torch.cuda.device(a.device):
        des = design(moments(a, t, groups, n_rep, c), plans)
        sums = sweep(a, t, groups, tests, des["M"], des["K"], c).cpu().numpy()
        st, delta = des["status"].cpu().numpy(), des["delta"].cpu().numpy()
        bare = unfiltered_sums(a.cpu().numpy(), t, groups, [1 << h for h in range(n_rep)])
    return _pick_tables(sums.reshape(n_rep, len(rows), t.shape[1], SUMS), st.reshape(n_rep, len(rows)), delta.reshape(n_rep, len(rows)),
                        bare, rows, n_rep)


class PoseFilter(KN.JointAngles):
    """A filtered pose per window, behind any of the four decoders or a `CommandGate`, with the calling surface of
    `JointAngles` (`push`, `push_packed`, `apply`, `state`, `reset`, `set_model`): per stream one steady-state Kalman filter on
    the device that reads the tail inputs every push leaves in the decoder's workspace (cp_online_kf_*; one launch more per
    push) and reports per window `raw` (M, D) f32, the regression itself (`JointAngles`' bits), `filtered` (M, D) f32, `pose`
    (M, D) int32, the bounded, rate-limited level of every joint out of 4096, and `angle` (M, D) f32.  Behind a gate the gate's
    `command` is the class input: while it is "none" the hand returns to its resting pose and the filter keeps tracking.

    fit: the `PoseFit` of the readout; model: a `FilterFit` (its plan 0 goes to every stream), or None: `set_model` /
    `FilterFit.install` later.  rate: the largest change of a level per window, 1..4096."""

    def __init__(self, source, fit: Optional[KN.PoseFit] = None, model: Optional[FilterFit] = None, rate: int = ONE):
        KN.JointAngles.__init__(self, source, None, 1, rate)
        self._cfg = _lib.cp_online_kf_config()
        self._cfg.rate = KN._check_stage(1, rate)[1]
        self.fit = fit
        if model is not None:
            if fit is not None and model.pose is not fit:
                raise ValueError("the filter was fitted behind another PoseFit")
            for s in range(self.n_streams):
                model.install(self, 0, s if self.multi else None)

    def set_model(self, *args):
        """set_model(W, b, lo, span, rest, M, K) on a single-stream source, set_model(stream, W, b, lo, span, rest, M, K) on a
        multi-stream one: the readout as `JointAngles.set_model` takes it and the filter's M (2D, 2D) and K (2D, D) f32 (on the
        GPU they never visit the host).  That stream starts again: not started, pose 0."""
        import torch
        if len(args) != (8 if self.multi else 7):
            raise TypeError("set_model(stream, W, b, lo, span, rest, M, K) on a multi-stream source, set_model(W, b, lo, span, rest, M, K) "
                            "otherwise")
        s = self._index(args[0]) if self.multi else 0
        W, b, lo, span, rest, M, K = args[-7:]
        W = torch.as_tensor(W, dtype=torch.float32).to(self.device).contiguous()
        b = torch.as_tensor(b, dtype=torch.float32).to(self.device).contiguous()
        M = torch.as_tensor(M, dtype=torch.float32).to(self.device).contiguous()
        K = torch.as_tensor(K, dtype=torch.float32).to(self.device).contiguous()
        if W.dim() != 2 or W.shape[1] != F or not 1 <= W.shape[0] <= MAX_JOINTS or tuple(b.shape) != (W.shape[0],):
            raise ValueError(f"W (D, 512) and b (D,) with D in 1..{MAX_JOINTS}")
        d = int(W.shape[0])
        if tuple(M.shape) != (2 * d, 2 * d) or tuple(K.shape) != (2 * d, d):
            raise ValueError(f"M (2D, 2D) and K (2D, D) with D = {d}")
        if W.data_ptr() % 16:
            W = W.clone()
        lo, span, rest = KN._check_limits(lo, span, rest, d)
        args = self._args()
        i = C.POINTER(C.c_int32)
        _lib.check(self.lib.cp_online_kf_set_model(*args, s, W.data_ptr(), b.data_ptr(), d, _fptr(lo), _fptr(span), rest.ctypes.data_as(i),
                                                   M.data_ptr(), K.data_ptr(), self._stream()), "cp_online_kf_set_model")
        self._joints[s] = d

    # ------------------------------------------------------------------ the device side
    def _args(self):
        import torch
        if self.ws is None:
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_kf_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return C.byref(self._cfg), self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_reset(self, s: int):
        args = self._args()
        _lib.check(self.lib.cp_online_kf_reset(*args, s, self._stream()), "cp_online_kf_reset")

    def _dev_push(self, tail, ldt: int, cls, row0: np.ndarray, m: np.ndarray, rows: int):
        """one launch over `rows` packed rows of tail -> raw, filtered, pose, angle (rows, 32)"""
        import torch
        from .online import _rows_on_device
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.device)
        fl = torch.empty(3, rows, MAX_JOINTS, dtype=torch.float32, device=self.device)
        pose = torch.empty(rows, MAX_JOINTS, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.cp_online_kf_push(*args, tail.data_ptr(), R._dtype_code(tail), ldt, None if cls is None else cls.data_ptr(),
                                              rm[0].data_ptr(), rm[1].data_ptr(), rows, fl[0].data_ptr(), fl[1].data_ptr(), pose.data_ptr(),
                                              fl[2].data_ptr(), self._stream()), "cp_online_kf_push")
        return fl[0], fl[1], pose, fl[2]

    def _empty(self):
        import torch
        return tuple(torch.empty(0, MAX_JOINTS, dtype=dt, device=self.device)
                     for dt in (torch.float32, torch.float32, torch.int32, torch.float32))

    def _join(self, outs):
        """per-launch per-stream (raw, filtered, pose, angle) -> per stream"""
        import torch
        if len(outs) == 1:
            return outs[0]
        if not outs:
            return self._split(self._empty(), np.zeros(self.n_streams, dtype=np.int64))
        return [tuple(torch.cat([o[s][i] for o in outs]) for i in range(4)) for s in range(self.n_streams)]

    def _behind(self, res_per_stream, row0: np.ndarray, m: np.ndarray):
        if int(m.sum()) == 0:
            return self._split(self._empty(), m)
        return KN.JointAngles._behind(self, res_per_stream, row0, m)

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back (this waits for the device; a test and debugging aid): joints
        (0: no model), started, x (2D,) f32 and out (D,), the pose.  The layout is that of OkfState (csrc/online_kalman.cuh): int32
        D, started, 6 unused, f32 x[64], int32 out[32], rest[32], f32 lo[32], span[32], b[32], c[32], M[64][64], K[64][32],
        W[32][512]."""
        import torch
        s = self._index(stream)
        if self.ws is None:
            return dict(joints=0, started=False, x=np.zeros(0, dtype=np.float32), out=np.zeros(0, dtype=np.int64))
        w = self.ws[:self.n_streams * _STATE_WORDS * 4].view(torch.int32).reshape(self.n_streams, _STATE_WORDS)[s]
        w = w[:_STATE_HEAD + 3 * MAX_JOINTS].cpu().numpy()
        d = int(w[0])
        x = w[_STATE_HEAD:_STATE_HEAD + 2 * MAX_JOINTS].view(np.float32)
        return dict(joints=d, started=bool(w[1]), x=x[:2 * d].copy(), out=w[_STATE_HEAD + 2 * MAX_JOINTS:][:d].astype(np.int64))
