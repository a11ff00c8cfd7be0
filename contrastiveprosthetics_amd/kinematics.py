"""Joint-angle decoding: a ridge pose readout behind the decoders.

Everything else the online chain emits is a class, or one level beside a class.  This module emits a pose: the recordings the
project was built around carry a data glove sampled alongside the sEMG, and here its angles are regressed linearly from the
tail inputs u (fc7's output, 512 values per 10 ms window) in closed form, with a ridge penalty, by the normal equations
`readout` already solves.  A stage behind any of the four decoders (`JointAngles`) then turns the regression into a bounded,
smoothed, rate-limited pose per window and stream.  The device side is cp_online_tail_offset and cp_online_kin_*
(include/cpnative.h, csrc/online_kinematics.cuh) and cp_online_readout_solve; the functions named *_reference and
`JointReference` are the definitions, in numpy with every operation rounded on its own (no fused multiply-add, no BLAS, no
np.linalg), and the device equals them in every bit.

Targets (`window_targets`).  glove (n_samples, D) f32, 1 <= D <= 32.  The target of window k is the glove sample at the centre
of window k + lag: sample phase + 20 (k + lag) + WINDOW_EDGE; lag >= 0 in windows models the EMG leading the movement.  Windows
whose target runs past the end are unused; a target that is not finite is refused.

Moments (`moments_reference`): exactly `readout.moments_reference` with the window's own target row y_i in place of E^[slot_i].
x_i = [u_i, 1]; per group (repetition) r over its windows in window order, from 0, in float64:
G_r[a][b] += w_i * (x_ia * x_ib) and C_r[a][d] += w_i * (x_ia * y_id): the product of two f32 values is exact, then one rounded
multiply by w_i and one rounded add.  A window is used when its group is >= 0; the default weight is 1 / N_used.

Solve (`solve_reference`).  A plan is (group mask, ridge) as in `readout`; the solution is `readout.solve_reference` on the
joints in column blocks of 16, the last block padded with zeros (a zero right-hand side solves to zero).  W (D, 512) and b (D)
are rounded to f32 once; the status is the same for every block of a plan.

Pose matvec (`pose_reference`).  u widened exactly to f32, every operation a single f32 operation.  For joint d partial sum l of
64 takes the products W[d][l + 64 j] * u[l + 64 j], j = 0..7 ascending, from +0.0f: each product rounded, then added and rounded.
Then p[l] = p[l] + p[l + s] for l < s, s = 32, 16, 8, 4, 2, 1, and a_d = p[0] + b_d.

State machine (`JointReference`), one per stream, windows in order, levels integers out of 4096.  A stream's model is W, b,
lo[D], span[D] (> 0, finite) and rest[D] in 0..4096.  t = (a_d - lo_d) / span_d (correctly rounded); a NaN t gives q = rest_d,
else q = (int) rintf(fminf(fmaxf(t, 0), 1) * 4096); with a class input, a row whose class is < 0 ("none") gives q = rest_d.
q enters the joint's ring of `smooth` entries (1..64), s = floor(ring sum / entries); out_d moves towards s by at most `rate`
(1..4096) per window.  Per row raw = a (f32), pose = out (int32), angle = lo_d + ((float) out / 4096.f) * span_d (a multiply,
then an add).  With smooth = 1, rate = 4096 and no class input pose = q.

Score (`score_reference`).  Per (plan, joint), over the windows whose group is in the plan's test mask, in window order, in
float64 with every operation rounded on its own: n, sum y, sum y^2, sum p, sum p^2, sum y p, sum (p - y)^2 of the f32 values
widened.  `metrics` derives RMSE, R^2 and Pearson's r from the seven sums on the host.

Nothing here is claimed for real subjects: `kinematics_recording` is a synthetic person, and a linear map from these tail inputs
to a real hand's joint angles has not been measured.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from . import readout as R
from .constants import WINDOW_EDGE
from .track import _host

D_E = _lib.CP_D_E
F = R.F
X = R.X
STRIDE = _lib.CP_ONLINE_STRIDE
MAX_JOINTS = _lib.CP_ONLINE_KIN_MAX_JOINTS
MAX_SMOOTH = _lib.CP_ONLINE_KIN_MAX_SMOOTH
ONE = _lib.CP_ONLINE_KIN_ONE
SUMS = _lib.CP_ONLINE_KIN_SUMS
MAX_GROUPS = R.MAX_GROUPS
MAX_PLANS = R.MAX_PLANS
RIDGES = R.RIDGES
BLOCKS = MAX_JOINTS // D_E
_STATE_HEAD = 8                                                # OknState (csrc/online_kinematics.cuh): D, head, len, 5 unused,
_STATE_WORDS = _STATE_HEAD + 6 * MAX_JOINTS + MAX_SMOOTH * MAX_JOINTS + MAX_JOINTS * F    # out, sum, rest, lo, span, b, ring, W


# ---------------------------------------------------------------------------------------------------------------------------
# the definitions (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------
def _check_joints(d) -> int:
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 1 <= int(d) <= MAX_JOINTS:
        raise ValueError(f"the number of joints must be an integer in 1..{MAX_JOINTS}")
    return int(d)


def _glove_array(glove) -> np.ndarray:
    g = _host(glove)
    if g.ndim != 2 or g.dtype != np.float32 or not 1 <= g.shape[1] <= MAX_JOINTS:
        raise ValueError(f"glove must be (n_samples, D) float32 with D in 1..{MAX_JOINTS}")
    return g


def _check_lag(lag, phase) -> tuple:
    for name, v, top in (("lag", lag, 2 ** 20), ("phase", phase, STRIDE - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= top:
            raise ValueError(f"{name} must be an integer in 0..{top}")
    return int(lag), int(phase)


def window_targets(glove, phase: int = 0, lag: int = 0) -> np.ndarray:
    """y (n, D) f32: row k is the glove sample phase + 20 (k + lag) + WINDOW_EDGE, the centre of window k + lag, for the windows
    k = 0..n-1 of the recording whose target lies inside it (the windows from n on are unused).  glove (n_samples, D) f32 next
    to the raw samples; a target that is not finite is a ValueError.  Host only (numpy)."""
    g = _glove_array(glove)
    lag, phase = _check_lag(lag, phase)
    n_samples = int(g.shape[0])
    m = max(0, (n_samples - phase - 2 * WINDOW_EDGE - 1 + STRIDE) // STRIDE)          # online.windows_before
    first = phase + STRIDE * lag + WINDOW_EDGE
    n = min(m, max(0, (n_samples - 1 - first) // STRIDE + 1) if n_samples > first else 0)
    y = np.ascontiguousarray(g[first:first + STRIDE * n:STRIDE][:n])
    if not np.isfinite(y).all():
        raise ValueError("a glove target is not finite")
    return y


def _target_array(y, n: int) -> np.ndarray:
    t = _host(y)
    if t.ndim != 2 or t.shape[0] != n or t.dtype != np.float32 or not 1 <= t.shape[1] <= MAX_JOINTS:
        raise ValueError(f"targets must be ({n}, D) float32 with D in 1..{MAX_JOINTS}")
    if not np.isfinite(t).all():
        raise ValueError("a target is not finite")
    return np.ascontiguousarray(t)


def uniform_weights(groups, n: int) -> np.ndarray:
    """w_i (n,) float64: 1.0 / N_used on the windows whose group is >= 0 (all of them without groups), 0 elsewhere."""
    used = np.ones(n, dtype=bool) if groups is None else np.asarray(_host(groups)).astype(np.int64).reshape(-1) >= 0
    w = np.zeros(n)
    if used.any():
        w[used] = np.float64(1.0) / np.float64(used.sum())
    return w


def _weight_array(weights, groups, n: int) -> np.ndarray:
    if weights is None:
        return uniform_weights(groups, n)
    w = np.ascontiguousarray(np.asarray(_host(weights), dtype=np.float64).reshape(-1))
    if w.shape[0] != n or not np.isfinite(w).all():
        raise ValueError(f"weights must hold one finite value per window ({n})")
    return w


def moments_reference(u, y, weights=None, groups=None, n_groups: int = 1):
    """The definition of the moments (module docstring): (G (R, 513, 513) f64, C (R, 513, D) f64).  u (N, 512) stored tail
    inputs; y (N, D) f32 targets; weights (N,) f64, default uniform; groups (N,) or None (one group).  Host only (numpy)."""
    u64 = R._u_array(u)
    n = int(u64.shape[0])
    r_n = R._check_groups(n_groups)
    t = _target_array(y, n)
    g = R._group_array(groups, n, r_n)
    w = _weight_array(weights, groups, n)
    t64 = t.astype(np.float64)
    d = int(t.shape[1])
    G, Cm = np.zeros((r_n, X, X)), np.zeros((r_n, X, d))
    x = np.ones(X)
    with np.errstate(all="ignore"):
        for i in np.nonzero(g >= 0)[0].tolist():               # window order; every += is one rounded add
            x[:F] = u64[i]
            G[g[i]] += w[i] * (x[:, None] * x[None, :])
            Cm[g[i]] += w[i] * (x[:, None] * t64[i][None, :])
    return G, Cm


def column_blocks(Cm) -> np.ndarray:
    """C (R, 513, D) -> (2, R, 513, 16) f64: the joints in column blocks of 16, padded with zeros (what the device writes and
    cp_online_readout_solve takes block by block)."""
    Cm = np.asarray(Cm, dtype=np.float64)
    out = np.zeros((BLOCKS, Cm.shape[0], X, D_E))
    for k in range(BLOCKS):
        part = Cm[:, :, D_E * k:D_E * (k + 1)]
        out[k, :, :, :part.shape[2]] = part
    return out


def solve_reference(G, Cm, plans, return_x: bool = False):
    """The definition of the solve (module docstring): (W (P, D, 512) f32, b (P, D) f32, status (P,) int32) from G (R, 513, 513)
    and C (R, 513, D) f64; plans as `readout.fit_reference` takes them.  return_x=True: also X (P, 513, D) f64, the solution
    before it is rounded to f32.  Host only (numpy)."""
    Cm = np.asarray(Cm, dtype=np.float64)
    d = _check_joints(int(Cm.shape[2]))
    blocks = column_blocks(Cm)
    Ws, bs, xs, status = [], [], [], None
    for k in range((d + D_E - 1) // D_E):
        W, b, st, x = R.solve_reference(G, blocks[k], plans, return_x=True)
        if status is not None and not np.array_equal(st, status):
            raise AssertionError("the status of a plan depends on its matrix alone")
        Ws.append(W), bs.append(b), xs.append(x)
        status = st
    out = (np.ascontiguousarray(np.concatenate(Ws, axis=1)[:, :d]), np.ascontiguousarray(np.concatenate(bs, axis=1)[:, :d]), status)
    return out + (np.ascontiguousarray(np.concatenate(xs, axis=2)[:, :, :d]),) if return_x else out


def fit_reference(u, y, plans=None, ridge=0.1, groups=None, n_groups: int = 1, weights=None) -> dict:
    """The definition of the fit (module docstring).  u (N, 512) stored tail inputs; y (N, D) f32 targets; groups (N,) in
    0..n_groups-1 or negative (not used), None: one group; plans: (training groups, ridge) pairs, default all groups for every
    value of `ridge`.  Returns a dict: W (P, D, 512) f32, b (P, D) f32, status (P,) int32, X (P, 513, D) f64 (the solution
    before rounding), G, C (R, 513, D), weights, masks, ridges.  Host only (numpy)."""
    r_n = R._check_groups(n_groups)
    if plans is None:
        plans = [((1 << r_n) - 1, lam) for lam in np.asarray(ridge, dtype=np.float64).reshape(-1).tolist()]
    masks, ridges = R._plan_table(plans, r_n)
    n = int(R._u_array(u).shape[0])
    w = _weight_array(weights, groups, n)
    G, Cm = moments_reference(u, y, w, groups, r_n)
    W, b, status, xs = solve_reference(G, Cm, plans, return_x=True)
    return dict(W=W, b=b, status=status, X=xs, G=G, C=Cm, weights=w, masks=masks, ridges=ridges)


def _model_arrays(W, b):
    W32, b32 = np.array(_host(W), dtype=np.float32), np.array(_host(b), dtype=np.float32)
    if W32.ndim != 2 or W32.shape[1] != F or not 1 <= W32.shape[0] <= MAX_JOINTS or b32.shape != (W32.shape[0],):
        raise ValueError(f"W (D, 512) and b (D,) with D in 1..{MAX_JOINTS}")
    return W32, b32


def pose_reference(u, W, b) -> np.ndarray:
    """The definition of the pose matvec (module docstring): u (n, 512) stored tail inputs, W (D, 512) f32, b (D,) f32 -> a
    (n, D) f32.  Host only (numpy)."""
    u32 = R._u_array(u).astype(np.float32)
    W32, b32 = _model_arrays(W, b)
    with np.errstate(all="ignore"):
        p = np.zeros((u32.shape[0], W32.shape[0], 64), dtype=np.float32)
        for j in range(F // 64):
            t = W32[None, :, 64 * j:64 * j + 64] * u32[:, None, 64 * j:64 * j + 64]
            p = p + t
        s = 32
        while s:
            p = p[:, :, :s] + p[:, :, s:2 * s]
            s //= 2
        return p[:, :, 0] + b32[None, :]


def _check_limits(lo, span, rest, d: int):
    lo32, span32 = np.array(_host(lo), dtype=np.float32).reshape(-1), np.array(_host(span), dtype=np.float32).reshape(-1)
    rest32 = np.asarray(_host(rest)).reshape(-1)
    if lo32.shape != (d,) or span32.shape != (d,) or rest32.shape != (d,):
        raise ValueError(f"lo, span and rest hold one value per joint ({d})")
    if not np.isfinite(lo32).all():
        raise ValueError("lo must be finite")
    if not (np.isfinite(span32) & (span32 > 0)).all():
        raise ValueError("span must be finite and > 0")
    if rest32.dtype.kind not in "iu" or (rest32 < 0).any() or (rest32 > ONE).any():
        raise ValueError(f"rest must hold integers in 0..{ONE}")
    return lo32, span32, rest32.astype(np.int32)


def _check_stage(smooth, rate):
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or not 1 <= int(smooth) <= MAX_SMOOTH:
        raise ValueError(f"smooth must be an int in 1..{MAX_SMOOTH}")
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or not 1 <= int(rate) <= ONE:
        raise ValueError(f"rate must be an int in 1..{ONE}")
    return int(smooth), int(rate)


class JointReference:
    """The definition of one stream's state machine (module docstring).  W (D, 512), b (D,), lo, span (D,) f32 and rest (D,)
    integers in 0..4096; smooth 1..64, rate 1..4096.  `push(u, cls=None)` takes the next rows (n, 512) and optionally their
    classes (n,) (< 0: none) and returns (raw (n, D) f32, pose (n, D) int32, angle (n, D) f32); the state carries over, so any
    cut of the rows into calls gives the same rows.  `q` holds the q of the rows of the last call.  Host only (numpy)."""

    def __init__(self, W, b, lo, span, rest, smooth: int = 5, rate: int = ONE):
        self.W, self.b = _model_arrays(W, b)
        self.D = int(self.W.shape[0])
        self.lo, self.span, self.rest = _check_limits(lo, span, rest, self.D)
        self.smooth, self.rate = _check_stage(smooth, rate)
        self.events = set()                                    # what has happened so far: nan, clamp_low, clamp_high, none,
        self.reset()                                           # ring_filling, rise_limited, fall_limited (a test aid)

    def reset(self):
        self.head, self.len = 0, 0
        self.ring = np.zeros((self.smooth, self.D), dtype=np.int64)
        self.sum = np.zeros(self.D, dtype=np.int64)
        self.out = np.zeros(self.D, dtype=np.int64)
        self.q = np.zeros((0, self.D), dtype=np.int64)

    def push(self, u, cls=None):
        a = pose_reference(u, self.W, self.b)
        n = int(a.shape[0])
        c = None
        if cls is not None:
            c = np.asarray(_host(cls)).astype(np.int64).reshape(-1)
            if c.shape[0] != n:
                raise ValueError(f"cls must hold one entry per row ({n})")
        pose, angle, qs = np.zeros((n, self.D), dtype=np.int32), np.zeros((n, self.D), dtype=np.float32), np.zeros((n, self.D), dtype=np.int64)
        one = np.float32(ONE)
        with np.errstate(all="ignore"):
            for i in range(n):
                t = (a[i] - self.lo) / self.span               # f32, each rounded on its own
                f = np.minimum(np.maximum(np.where(np.isnan(t), np.float32(0), t), np.float32(0)), np.float32(1))
                q = np.rint(f * one).astype(np.int64)
                q = np.where(np.isnan(t), self.rest, q)
                if c is not None and c[i] < 0:
                    q = self.rest.astype(np.int64)
                for name, hit in (("nan", np.isnan(t).any()), ("clamp_low", (t < 0).any()), ("clamp_high", (t > 1).any()),
                                  ("none", c is not None and c[i] < 0), ("ring_filling", self.len < self.smooth)):
                    if hit:
                        self.events.add(name)
                if self.len == self.smooth:
                    self.sum = self.sum - self.ring[self.head]
                else:
                    self.len += 1
                self.sum = self.sum + q
                self.ring[self.head] = q
                self.head = (self.head + 1) % self.smooth
                s = self.sum // self.len
                if (s > self.out + self.rate).any():
                    self.events.add("rise_limited")
                if (s < self.out - self.rate).any():
                    self.events.add("fall_limited")
                self.out = np.where(s > self.out, np.minimum(self.out + self.rate, s), np.maximum(self.out - self.rate, s))
                pose[i], qs[i] = self.out, q
                lvl = self.out.astype(np.float32) / one
                scaled = lvl * self.span
                angle[i] = self.lo + scaled
        self.q = qs
        return a, pose, angle

    def state(self) -> dict:
        """out (D,) and ring, the (entries, D) q values from the oldest to the newest, as `JointAngles.state` reports them"""
        at = [(self.head - self.len + i) % self.smooth for i in range(self.len)]
        return dict(out=self.out.astype(np.int64).copy(), ring=self.ring[at].astype(np.int64).reshape(self.len, self.D))


def _mask_array(test_masks, n_groups: int = MAX_GROUPS) -> np.ndarray:
    m = np.asarray(_host(test_masks)).astype(np.int64).reshape(-1)
    if m.shape[0] > MAX_PLANS or (m < 0).any() or (m >> n_groups).any():
        raise ValueError(f"test masks: at most {MAX_PLANS} bit masks of groups 0..{n_groups - 1}")
    return m


def score_reference(pred, y, groups, test_masks) -> np.ndarray:
    """The definition of the score (module docstring): pred (P, N, D) f32, y (N, D) f32, groups (N,), test_masks (P,) bit masks
    of groups -> sums (P, D, 7) f64: n, sum y, sum y^2, sum p, sum p^2, sum y p, sum (p - y)^2.  Host only (numpy)."""
    p32 = np.array(_host(pred), dtype=np.float32)
    t = np.array(_host(y), dtype=np.float32)
    if p32.ndim != 3 or t.ndim != 2 or p32.shape[1:] != t.shape:
        raise ValueError("pred (P, N, D) and y (N, D)")
    g = np.asarray(_host(groups)).astype(np.int64).reshape(-1)
    masks = _mask_array(test_masks)
    if g.shape[0] != t.shape[0] or masks.shape[0] != p32.shape[0]:
        raise ValueError("one group per row and one test mask per plan")
    out = np.zeros((p32.shape[0], t.shape[1], SUMS))
    zero = np.zeros((1, t.shape[1]))
    with np.errstate(all="ignore"):
        for k in range(p32.shape[0]):
            sel = (g >= 0) & (g < MAX_GROUPS) & (((int(masks[k]) >> np.clip(g, 0, 62)) & 1) == 1)
            yy, pp = t[sel].astype(np.float64), p32[k][sel].astype(np.float64)
            e = pp - yy
            for j, v in enumerate((np.ones_like(yy), yy, yy * yy, pp, pp * pp, yy * pp, e * e)):
                out[k, :, j] = np.cumsum(np.concatenate([zero, v]), axis=0)[-1]        # sequential, from +0.0
    return out


def metrics(sums) -> dict:
    """RMSE, R^2 and Pearson's r per (..., joint) from sums (..., D, 7) f64, and their means over the joints (rmse_mean,
    r2_mean, r_mean, over the joints with windows); NaN where they are not defined.  Host only (numpy, float64)."""
    s = np.asarray(_host(sums), dtype=np.float64)
    n, sy, syy, sp, spp, syp, see = (s[..., j] for j in range(SUMS))
    with np.errstate(all="ignore"):
        rmse = np.sqrt(see / n)
        vy, vp = syy - sy * sy / n, spp - sp * sp / n
        r2 = 1.0 - see / vy
        r = (syp - sy * sp / n) / np.sqrt(vy * vp)
        rmse, r2, r = (np.where(n > 0, v, np.nan) for v in (rmse, r2, r))

        def mean(v):                                           # over the joints where it is defined; NaN if there is none
            has = np.isfinite(v)
            return np.where(has, v, 0.0).sum(axis=-1) / has.sum(axis=-1)

        return dict(rmse=rmse, r2=r2, r=r, rmse_mean=mean(rmse), r2_mean=mean(r2), r_mean=mean(r))


def limits(y, cls=None, rest_class: int = 0, low: float = 1.0, high: float = 99.0):
    """(lo (D,) f32, span (D,) f32, rest (D,) int32) of a stage from training targets y (N, D) f32: lo and hi the `low`-th and
    `high`-th percentile per joint, span = hi - lo (at least 1e-6 of the larger bound, so it is > 0); rest the level (out of 4096)
    of the mean target over the windows whose class is `rest_class` when cls (N,) is given and has such windows, else of the
    median target.  Host only (numpy)."""
    t = np.array(_host(y), dtype=np.float32)
    if t.ndim != 2 or t.shape[0] < 1:
        raise ValueError("limits need at least one target row")
    lo = np.percentile(t.astype(np.float64), low, axis=0)
    hi = np.percentile(t.astype(np.float64), high, axis=0)
    span = np.maximum(hi - lo, 1e-6 * np.maximum(1.0, np.maximum(np.abs(lo), np.abs(hi))))
    at = np.median(t.astype(np.float64), axis=0)
    if cls is not None:
        c = np.asarray(_host(cls)).reshape(-1)
        if c.shape[0] != t.shape[0]:
            raise ValueError("cls must hold one entry per target row")
        if (c == rest_class).any():
            at = t[c == rest_class].astype(np.float64).mean(axis=0)
    rest = np.clip(np.rint((at - lo) / span * ONE), 0, ONE).astype(np.int32)
    return lo.astype(np.float32), np.maximum(span.astype(np.float32), np.float32(1e-30)), rest


def kinematics_recording(k: int = 6, reps: int = 3, segment: int = 30, joints: int = 20, delay: int = 2, seed: int = 0,
                         noise: float = 0.3, phase: int = 0) -> dict:
    """A synthetic person for tests and measurements; nothing about real subjects.  Class c has a pose of `joints` angles in
    degrees; the cue walks through rest (class 0) and the classes once per repetition, `segment` windows each, and the joint
    angles follow the cued pose through a first-order lag.  The tail inputs are a noisy linear image of the angles `delay`
    windows LATER (the EMG leads the movement), passed through max(., 0).  Returns a dict: u (N, 512) f32; y (N, joints) f32,
    the angle at each window's centre; glove (n_samples, joints) f32 at the raw rate with `window_targets(glove, phase)` == y;
    cls (N,) int64 the cued class (0: rest); rep (N,) int64 and n_rep; n_samples.  Host only; the same arrays for the same
    arguments."""
    rng = np.random.default_rng(seed)
    d = _check_joints(joints)
    poses = rng.uniform(5.0, 85.0, size=(k, d))
    poses[0] = rng.uniform(0.0, 10.0, size=d)
    cls, rep = [], []
    for r in range(reps):
        for c in range(k):
            cls += [c] * segment
            rep += [r] * segment
    cls, rep = np.array(cls, dtype=np.int64), np.array(rep, dtype=np.int64)
    n = int(cls.shape[0])
    ang = np.zeros((n + delay, d))
    cur = poses[0].copy()
    for i in range(n + delay):
        cur = cur + 0.25 * (poses[cls[min(i, n - 1)]] - cur)
        ang[i] = cur
    mix = rng.standard_normal((d, F)) / np.sqrt(d)
    lead = ang[delay:delay + n]                                # what the muscles already do at window i
    u = np.maximum((lead - 45.0) / 30.0 @ mix + 0.5 + noise * rng.standard_normal((n, F)), 0.0).astype(np.float32)
    y = ang[:n].astype(np.float32)
    n_samples = phase + STRIDE * (n - 1) + 2 * WINDOW_EDGE + 1
    glove = np.repeat(y, STRIDE, axis=0)
    glove = np.concatenate([np.repeat(y[:1], phase + WINDOW_EDGE, axis=0), glove])[:n_samples]
    glove = np.ascontiguousarray(glove)
    return dict(u=u, y=y, glove=glove, cls=cls, rep=rep, n_rep=int(reps), n_samples=int(n_samples))


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
def _device_targets(y, n: int, dev):
    import torch
    t = _target_array(y, n)
    return torch.from_numpy(t).to(dev), int(t.shape[1])


def moments(u, y, weights=None, groups=None, n_groups: int = 1):
    """`moments_reference` on the device (cp_online_kin_moments): u (N, 512) f32 or bf16 on the GPU; y (N, D) f32; the other
    arguments as the definition takes them, checked before the first launch.  Returns (G (R, 513, 513), C (2, R, 513, 16)) f64
    on the GPU: C in the column blocks of `column_blocks`."""
    import torch
    u = R._device_u(u)
    n, dev = int(u.shape[0]), u.device
    r_n = R._check_groups(n_groups)
    g = R._group_array(groups, n, r_n)
    w = _weight_array(weights, groups, n)
    lib = _lib.load()
    with torch.cuda.device(dev):
        y_d, d = _device_targets(y, n, dev)
        g_d, w_d = torch.from_numpy(g.astype(np.int32)).to(dev), torch.from_numpy(w).to(dev)
        G = torch.empty(r_n, X, X, dtype=torch.float64, device=dev)
        Cm = torch.empty(BLOCKS, r_n, X, D_E, dtype=torch.float64, device=dev)
        sc = R._scratch(lib, n, r_n, 1, dev)
        _lib.check(lib.cp_online_kin_moments(u.data_ptr() if n else None, R._dtype_code(u), n, g_d.data_ptr() if n else None,
                                             w_d.data_ptr() if n else None, y_d.data_ptr() if n else None, d, d, r_n, G.data_ptr(),
                                             Cm.data_ptr(), sc.data_ptr(), sc.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "cp_online_kin_moments")
    return G, Cm


def solve(G, Cm, plans, n_joints: int):
    """`solve_reference` on the device: cp_online_readout_solve once per column block of C (2, R, 513, 16).  Returns (W
    (P, D, 512) f32, b (P, D) f32, status (P,) int32) on the GPU; nothing visits the host."""
    import torch
    d = _check_joints(n_joints)
    if not isinstance(Cm, torch.Tensor) or Cm.dim() != 4 or Cm.shape[0] != BLOCKS:
        raise ValueError("C (2, R, 513, 16) float64 on the GPU, as `moments` returns it")
    Ws, bs, status = [], [], None
    for k in range((d + D_E - 1) // D_E):
        W, b, status = R.solve(G, Cm[k], plans)
        Ws.append(W), bs.append(b)
    W = Ws[0] if len(Ws) == 1 else torch.cat(Ws, dim=1)
    b = bs[0] if len(bs) == 1 else torch.cat(bs, dim=1)
    return W[:, :d].contiguous(), b[:, :d].contiguous(), status


def _device_model(W, b, dev):
    import torch
    W = torch.as_tensor(W, dtype=torch.float32).to(dev).contiguous()
    b = torch.as_tensor(b, dtype=torch.float32).to(dev).contiguous()
    if W.dim() == 2:
        W, b = W[None], b[None]
    if W.dim() != 3 or W.shape[2] != F or not 1 <= W.shape[1] <= MAX_JOINTS or tuple(b.shape) != tuple(W.shape[:2]) \
            or W.shape[0] > MAX_PLANS:
        raise ValueError(f"W (P, D, 512) and b (P, D), D <= {MAX_JOINTS}, P <= {MAX_PLANS}")
    if W.data_ptr() % 16:
        W = W.clone()
    return W, b


def apply(u, W, b):
    """a (P, n, D) f32 on the GPU: `pose_reference` of u (n, 512) f32 or bf16 on the GPU under every W (P, D, 512), b (P, D)
    (cp_online_kin_apply): the stage's own matvec, so bit for bit the `raw` a `JointAngles` with that model emits."""
    import torch
    u = R._device_u(u)
    n, dev = int(u.shape[0]), u.device
    W, b = _device_model(W, b, dev)
    n_p, d = int(W.shape[0]), int(W.shape[1])
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.empty(n_p, n, d, dtype=torch.float32, device=dev)
        if n and n_p:
            _lib.check(lib.cp_online_kin_apply(u.data_ptr(), R._dtype_code(u), n, W.data_ptr(), b.data_ptr(), n_p, d, out.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), "cp_online_kin_apply")
    return out


def score(pred, y, groups, test_masks):
    """`score_reference` on the device (cp_online_kin_score): pred (P, N, D) f32 on the GPU, y (N, D) f32, groups (N,),
    test_masks (P,) -> sums (P, D, 7) f64 on the GPU."""
    import torch
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.float32 or pred.dim() != 3 or pred.device.type != "cuda":
        raise ValueError("pred must be a (P, N, D) float32 tensor on the GPU")
    pred = pred.contiguous()
    n_p, n, d = (int(v) for v in pred.shape)
    dev = pred.device
    masks = _mask_array(test_masks)
    g = np.asarray(_host(groups)).astype(np.int64).reshape(-1)
    if g.shape[0] != n or masks.shape[0] != n_p:
        raise ValueError("one group per row and one test mask per plan")
    lib = _lib.load()
    with torch.cuda.device(dev):
        y_d, dy = _device_targets(y, n, dev)
        if dy != d:
            raise ValueError("pred and y disagree on the number of joints")
        g_d = torch.from_numpy(np.clip(g, -1, MAX_GROUPS).astype(np.int32)).to(dev)
        sums = torch.zeros(n_p, d, SUMS, dtype=torch.float64, device=dev)
        if n_p:
            _lib.check(lib.cp_online_kin_score(pred.data_ptr() if n else None, y_d.data_ptr() if n else None, d,
                                               g_d.data_ptr() if n else None, (C.c_uint32 * n_p)(*masks.tolist()), n_p, n, d,
                                               sums.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cp_online_kin_score")
    return sums


class PoseFit:
    """What `fit_pose` found: W (P, D, 512) and b (P, D) f32 on the GPU, status (P,) int32 numpy (0, or j + 1 for a pivot that
    failed at column j: W and b of that plan are zero and it is never installed), plans, the list of (training groups as a sorted
    tuple, ridge), counts {group: windows used}, lo, span (D,) f32 and rest (D,) int32 (`limits` of the training targets), lag,
    and dtype, the compute dtype of the decoder whose tail inputs were fitted."""

    def __init__(self, W, b, status, plans, counts, lo, span, rest, lag: int = 0, dtype: str = "f32"):
        self.W, self.b = W, b
        self.status = np.asarray(status, dtype=np.int32).reshape(-1)
        self.plans, self.counts = list(plans), dict(counts)
        self.n_joints = int(W.shape[1])
        self.lo, self.span, self.rest = _check_limits(lo, span, rest, self.n_joints)
        self.lag, self.dtype = int(lag), dtype

    def _index(self, index) -> int:
        n = int(self.status.shape[0])
        if isinstance(index, bool) or not isinstance(index, (int, np.integer)) or not 0 <= int(index) < n:
            raise IndexError(f"index must be an int in 0..{n - 1}, got {index!r}")
        if self.status[int(index)] != 0:
            raise ValueError(f"plan {int(index)} (ridge {self.plans[int(index)][1]!r}) has no readout: its matrix is not positive "
                             f"definite (pivot {int(self.status[int(index)]) - 1}); raise the ridge")
        return int(index)

    def install(self, stage, index: int = 0, stream: Optional[int] = None):
        """Install plan `index` into a `JointAngles` stage (`stage.set_model`): on a multi-stream source into `stream`.  That
        stream of the stage restarts.  A plan whose status is not 0 is a ValueError."""
        i = self._index(index)
        if stage.multi:
            if stream is None:
                raise ValueError("stream= names the stream of a multi-stream source")
            stage.set_model(stream, self.W[i], self.b[i], self.lo, self.span, self.rest)
        else:
            if stream is not None:
                raise ValueError("stream= goes with a multi-stream source")
            stage.set_model(self.W[i], self.b[i], self.lo, self.span, self.rest)

    def apply(self, u_or_decoder, raw=None, stream: Optional[int] = None):
        """a (P, n, D) f32 on the GPU: every plan's readout applied to u (n, 512) tail inputs on the GPU, or to every window
        of the recording raw (n, 12) through `decoder` (a multi-stream one with `stream`): `PoseFit.apply(decoder, raw)`."""
        if raw is None:
            return apply(u_or_decoder, self.W, self.b)
        dec = u_or_decoder
        _, key = R._decoder_key(dec, stream)
        from .online import windows_before
        u = dec._recording_tail_inputs(key, raw, np.arange(windows_before(int(raw.shape[0]), dec.phase)))
        return apply(u, self.W, self.b)


def _recording(decoder, raw, glove, stream, who: str):
    """the checks `fit_pose` and `pick_pose` share -> (key, glove array, windows of the recording)"""
    from .online import _check_raw, windows_before
    _, key = R._decoder_key(decoder, stream)
    if not decoder._enroll_view(key)[2]:
        raise _lib.CpNativeError(f"an AdaBN model has no BatchNorm statistics: calibrate() first, then {who}()")
    _check_raw(raw)
    g = _glove_array(glove)
    if g.shape[0] != raw.shape[0]:
        raise ValueError(f"glove must hold one row per raw sample ({int(raw.shape[0])})")
    return key, g, windows_before(int(raw.shape[0]), decoder.phase)


def _rep_groups(rep, m: int, folds=None):
    """rep: None (one group), or (rep (M,), R) as `holdout.repetitions` gives it -> (groups (M,) int64, R), folded by `folds`"""
    if rep is None:
        return np.zeros(m, dtype=np.int64), 1
    rep_w, n_rep = rep
    g = np.asarray(_host(rep_w))
    if g.shape != (m,) or g.dtype.kind not in "iu":
        raise ValueError(f"rep must hold one integer entry per window of the recording ({m})")
    g, n_rep = g.astype(np.int64), int(n_rep)
    if folds is not None:
        if isinstance(folds, bool) or not isinstance(folds, (int, np.integer)) or not 1 <= int(folds) <= MAX_GROUPS:
            raise ValueError(f"folds must be an integer in 1..{MAX_GROUPS}")
        g, n_rep = np.where(g >= 0, g % int(folds), -1), min(n_rep, int(folds))
    R._check_groups(n_rep)
    if m and g.max() >= n_rep:
        raise ValueError(f"a repetition index must stay below the number of repetitions ({n_rep})")
    return np.maximum(g, -1), n_rep


def fit_pose(decoder, raw, glove, *, rep=None, ridge=0.1, plans=None, lag: int = 0, stream: Optional[int] = None, weights=None,
             labels=None, rest_label: int = 0) -> PoseFit:
    """A pose readout in closed form (module docstring).  decoder: any of the four online decoders (a multi-stream one with
    `stream`); raw (n, 12) f32 on the GPU and glove (n, D) f32, one row per raw sample (a stream of its own, read through the
    decoder's electrode map and embedded by its own encoder, the adaptive forms with their statistics frozen).  rep: (rep (M,),
    R) as `holdout.repetitions` gives it, one entry per window (negative: not used), default one group; ridge: a float or a
    list; plans: a list of (training repetitions, ridge), default all repetitions for every ridge; lag >= 0 in windows;
    weights (M,) f64, default uniform over the used windows.  labels (n,) per raw sample, optional: the windows labelled
    `rest_label` give the stage's resting pose.  lo, span and rest are `limits` of the used targets, computed on the host.

    Fit AFTER `calibrate`: calibration moves the BatchNorm statistics and with them the tail inputs, so a readout fitted
    before it no longer matches what a push computes.  The decoder is not changed.  One host synchronisation: the copy of
    `status`."""
    import torch
    key, g, m = _recording(decoder, raw, glove, stream, "fit_pose")
    y = window_targets(g, decoder.phase, lag)
    n = int(y.shape[0])
    if n < 1:
        raise ValueError("the recording has no window with a target")
    groups, n_rep = _rep_groups(rep, m)
    groups = groups[:n]
    masks, ridges = R._plan_table(R._default_plans(ridge, plans, n_rep), n_rep)
    if masks.shape[0] < 1:
        raise ValueError("at least one plan")
    if not (groups >= 0).any():
        raise ValueError("no window of the recording is used")
    w = _weight_array(None if weights is None else np.asarray(_host(weights), dtype=np.float64).reshape(-1)[:n], groups, n)
    cls = None
    if labels is not None:
        from .online import _sample_labels, window_labels
        cls = window_labels(_sample_labels(labels, raw.shape[0]), decoder.phase)[:n][groups >= 0]
    lo, span, rest = limits(y[groups >= 0], cls, rest_label)
    # ---- everything is checked: from here on work is enqueued
    u = decoder._recording_tail_inputs(key, raw, np.arange(n))
    with torch.cuda.device(decoder.device):
        G, Cm = moments(u, y, w, groups, n_rep)
        W, b, status = solve(G, Cm, list(zip(masks.tolist(), ridges.tolist())), int(y.shape[1]))
        st = status.cpu().numpy()
    named = [(tuple(r for r in range(n_rep) if (int(mk) >> r) & 1), float(l)) for mk, l in zip(masks.tolist(), ridges.tolist())]
    counts = {int(r): int((groups == r).sum()) for r in range(n_rep)}
    return PoseFit(W, b, st, named, counts, lo, span, rest, lag, decoder.dtype)


def _pick_tables(sums, status, lam: np.ndarray, lags, n_rep: int) -> dict:
    """the tables of `pick_pose` from sums (L, R, T, D, 7) of the held-out folds and status (L, R, T)"""
    sums = np.asarray(sums, dtype=np.float64)
    n_l, n_t = int(sums.shape[0]), int(lam.shape[0])
    total = np.zeros(sums.shape[:1] + sums.shape[2:])
    for h in range(n_rep):                                     # fold order, one rounded add each
        total = total + sums[:, h]
    ok = (np.asarray(status).reshape(n_l, n_rep, n_t) == 0).all(axis=1)
    met = metrics(total)
    best = None
    for li in range(n_l):                                      # the smallest mean held-out RMSE, the larger ridge among equals
        for t in range(n_t):
            v = met["rmse_mean"][li, t]
            if not ok[li, t] or not np.isfinite(v):
                continue
            if best is None or (v, -lam[t]) < (met["rmse_mean"][best], -lam[best[1]]):
                best = (li, t)
    out = dict(ridges=lam, lags=np.asarray(list(lags), dtype=np.int64), sums=total, fold_sums=sums, ok=ok, n_rep=n_rep, best=best,
               ridge=None if best is None else float(lam[best[1]]), lag=None if best is None else int(list(lags)[best[0]]))
    out.update(met)
    return out


def _check_pick(ridges, lags, n_rep: int):
    lam = R._check_ridges(ridges)
    lags = [_check_lag(l, 0)[0] for l in lags]
    if not lags:
        raise ValueError("lags must hold at least one value")
    if n_rep < 2:
        raise ValueError("pick_pose needs at least two repetitions")
    if n_rep * lam.shape[0] > MAX_PLANS:
        raise ValueError(f"folds x ridges must stay within {MAX_PLANS} plans")
    return lam, lags


def _pick_plans(n_rep: int, lam: np.ndarray):
    plans = [(tuple(r for r in range(n_rep) if r != h), float(l)) for h in range(n_rep) for l in lam.tolist()]
    tests = np.array([1 << h for h in range(n_rep) for _ in lam.tolist()], dtype=np.int64)
    return plans, tests


def pick_pose_reference(u, glove, rep, ridges=RIDGES, lags=(0,), folds=None, phase: int = 0) -> dict:
    """`pick_pose` on the definitions alone (`window_targets`, `fit_reference`, `pose_reference`, `score_reference`): u (M, 512)
    the tail inputs of every window of the recording.  Host only (numpy)."""
    u64 = R._u_array(u)
    m = int(u64.shape[0])
    groups, n_rep = _rep_groups(rep, m, folds)
    lam, lags = _check_pick(ridges, lags, n_rep)
    plans, tests = _pick_plans(n_rep, lam)
    sums, status = [], []
    for lag in lags:
        y = window_targets(glove, phase, lag)
        n = int(y.shape[0])
        fit = fit_reference(u64[:n].astype(np.float32), y, plans, groups=groups[:n], n_groups=n_rep)
        pred = np.stack([pose_reference(u64[:n].astype(np.float32), fit["W"][p], fit["b"][p]) for p in range(len(plans))])
        sums.append(score_reference(pred, y, groups[:n], tests).reshape(n_rep, lam.shape[0], y.shape[1], SUMS))
        status.append(fit["status"].reshape(n_rep, lam.shape[0]))
    return _pick_tables(np.stack(sums), np.stack(status), lam, lags, n_rep)


def pick_pose_inputs(u, glove, rep, ridges=RIDGES, lags=(0,), folds=None, phase: int = 0) -> dict:
    """`pick_pose` behind the encoder: u (M, 512) f32 or bf16 on the GPU, the tail inputs of every window of the recording;
    glove (n_samples, D) f32.  Returns what `pick_pose` returns."""
    import torch
    u = R._device_u(u)
    m, dev = int(u.shape[0]), u.device
    g = _glove_array(glove)
    groups, n_rep = _rep_groups(rep, m, folds)
    lam, lags = _check_pick(ridges, lags, n_rep)
    plans, tests = _pick_plans(n_rep, lam)
    ys = [window_targets(g, phase, lag) for lag in lags]
    if any(y.shape[0] < 1 or y.shape[0] > m for y in ys):
        raise ValueError("glove and the tail inputs disagree on the windows of the recording")
    sums, status = [], []
    with torch.cuda.device(dev):
        for y in ys:
            n = int(y.shape[0])
            G, Cm = moments(u[:n], y, None, groups[:n], n_rep)
            W, b, st = solve(G, Cm, plans, int(y.shape[1]))
            sums.append(score(apply(u[:n], W, b), y, groups[:n], tests))
            status.append(st)
        sums = torch.stack(sums).cpu().numpy().reshape(len(lags), n_rep, lam.shape[0], g.shape[1], SUMS)
        status = torch.stack(status).cpu().numpy().reshape(len(lags), n_rep, lam.shape[0])
    return _pick_tables(sums, status, lam, lags, n_rep)


def pick_pose(decoder, raw, glove, rep, ridges=RIDGES, lags=(0,), folds=None, stream: Optional[int] = None) -> dict:
    """Which ridge and lag predict the pose of repetitions they have not seen best?  decoder, raw and glove as `fit_pose` takes
    them; rep: (rep (M,), R) per window (`holdout.repetitions`), folded to rep % folds with folds=.  Per lag and fold h: the fit
    on the other repetitions for every ridge (one cp_online_readout_solve per column block), the device apply on the whole
    recording and the device score on repetition h.

    Returns a dict: ridges (T,) f64, lags (L,) int64; sums (L, T, D, 7) f64, the held-out sums of the folds added in fold
    order, and fold_sums (L, R, T, D, 7); ok (L, T), False where a fold's matrix failed to factor; rmse, r2, r (L, T, D) and
    rmse_mean, r2_mean, r_mean (L, T) from `metrics`; best (lag index, ridge index) with the smallest mean held-out RMSE, the
    larger ridge among equals (None if none is valid); ridge, lag, n_rep.  The decoder is left as it was: nothing it holds is
    written (the recording is embedded by cp_online_*tail_inputs into buffers of its own)."""
    key, g, m = _recording(decoder, raw, glove, stream, "pick_pose")
    groups, n_rep = _rep_groups(rep, m, folds)
    _check_pick(ridges, lags, n_rep)
    u = decoder._recording_tail_inputs(key, raw, np.arange(m))
    return pick_pose_inputs(u, g, (groups, n_rep), ridges, lags, None, decoder.phase)


class JointAngles:
    """A pose per window, behind any of the four decoders or a `CommandGate`: per stream one state machine on the device that
    reads the tail inputs every push leaves in the decoder's workspace (`decoder.tail_view()`; include/cpnative.h,
    cp_online_kin_*; one launch more per push, nothing is copied to the host) and reports per window `raw` (M, D) f32, the
    regression itself, `pose` (M, D) int32, the bounded, smoothed, rate-limited level of every joint out of 4096, and `angle`
    (M, D) f32, that level in the glove's units.  Behind a gate the gate's `command` is the class input: while it is "none"
    the hand returns to its resting pose.

    fit: a `PoseFit` (its plan 0 goes to every stream), or None: `set_model` / `PoseFit.install` later.  smooth: ring length
    1..64, fixed at construction; rate: the largest change of a level per window, 1..4096.  A push of more windows than the
    decoder runs in one chain of launches is cut on the host so that every chain's tail inputs are read before the next one
    overwrites them.  A push or reset of the source behind the stage's back makes the next `push` raise `CpNativeError`."""

    def __init__(self, source, fit: Optional[PoseFit] = None, smooth: int = 5, rate: int = ONE):
        from .online import CommandGate
        self.gate = source if isinstance(source, CommandGate) else None
        self.source = source
        self.decoder = source.decoder if self.gate is not None else source
        for name in ("class_ids", "n_seen", "push", "tail_view"):
            if not hasattr(self.decoder, name):
                raise TypeError("JointAngles wraps a CommandGate, an OnlineDecoder, MultiStreamDecoder or AdaptiveMultiStreamDecoder")
        self.multi = isinstance(self.decoder.class_ids, (list, tuple))
        self.n_streams = len(self.decoder.class_ids) if self.multi else 1
        self.smooth, rate = _check_stage(smooth, rate)
        self._cfg = _lib.cp_online_kin_config()
        self._cfg.smooth, self._cfg.rate = self.smooth, rate
        self.device = self.decoder.device
        self.ws = None                                         # allocated with the first launch
        self._rows_cache = {}
        self._tail = None                                      # the decoder's tail_view(), taken with the first push
        self._joints = [0] * self.n_streams
        self._left = self._seen_now()
        if fit is not None:
            for s in range(self.n_streams):
                fit.install(self, 0, s if self.multi else None)

    # ------------------------------------------------------------------ settings
    @property
    def rate(self) -> int:
        return int(self._cfg.rate)

    def set(self, **kw):
        """Change rate from the next window on (smooth is fixed at construction: the ring is laid out by it)."""
        for k, v in kw.items():
            if k == "smooth":
                raise ValueError("smooth is fixed at construction: the ring is laid out by it")
            if k != "rate":
                raise TypeError(f"set() takes rate, not {k!r}")
            self._cfg.rate = _check_stage(self.smooth, v)[1]

    def _index(self, stream) -> int:
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {stream!r}")
        return int(stream)

    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def set_model(self, *args):
        """set_model(W, b, lo, span, rest) on a single-stream source, set_model(stream, W, b, lo, span, rest) on a multi-stream
        one: W (D, 512) and b (D,) f32 (on the GPU they never visit the host), lo, span (D,) f32 and rest (D,) integers in
        0..4096.  That stream starts again: ring empty, pose 0."""
        import torch
        if len(args) != (6 if self.multi else 5):
            raise TypeError("set_model(stream, W, b, lo, span, rest) on a multi-stream source, set_model(W, b, lo, span, rest) otherwise")
        s = self._index(args[0]) if self.multi else 0
        W, b, lo, span, rest = args[-5:]
        W = torch.as_tensor(W, dtype=torch.float32).to(self.device).contiguous()
        b = torch.as_tensor(b, dtype=torch.float32).to(self.device).contiguous()
        if W.dim() != 2 or W.shape[1] != F or not 1 <= W.shape[0] <= MAX_JOINTS or tuple(b.shape) != (W.shape[0],):
            raise ValueError(f"W (D, 512) and b (D,) with D in 1..{MAX_JOINTS}")
        if W.data_ptr() % 16:
            W = W.clone()
        d = int(W.shape[0])
        lo, span, rest = _check_limits(lo, span, rest, d)
        args = self._args()
        f, i = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _lib.check(self.lib.cp_online_kin_set_model(*args, s, W.data_ptr(), b.data_ptr(), d, lo.ctypes.data_as(f), span.ctypes.data_as(f),
                                                    rest.ctypes.data_as(i), self._stream()), "cp_online_kin_set_model")
        self._joints[s] = d

    # ------------------------------------------------------------------ the device side
    def _args(self):
        import torch
        if self.ws is None:
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_kin_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return C.byref(self._cfg), self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_reset(self, s: int):
        args = self._args()
        _lib.check(self.lib.cp_online_kin_reset(*args, s, self._stream()), "cp_online_kin_reset")

    def _dev_push(self, tail, ldt: int, cls, row0: np.ndarray, m: np.ndarray, rows: int):
        """one launch over `rows` packed rows of tail -> raw, pose, angle (rows, 32)"""
        import torch
        from .online import _rows_on_device
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.device)
        ra = torch.empty(2, rows, MAX_JOINTS, dtype=torch.float32, device=self.device)
        pose = torch.empty(rows, MAX_JOINTS, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.cp_online_kin_push(*args, tail.data_ptr(), R._dtype_code(tail), ldt, None if cls is None else cls.data_ptr(),
                                               rm[0].data_ptr(), rm[1].data_ptr(), rows, ra[0].data_ptr(), pose.data_ptr(),
                                               ra[1].data_ptr(), self._stream()), "cp_online_kin_push")
        return ra[0], pose, ra[1]

    def _split(self, outs, m: np.ndarray):
        """raw, pose, angle (rows, 32) of one launch -> per stream (raw, pose, angle) (M_s, D_s)"""
        ml = m.tolist()
        ds = {self._joints[s] for s, n in enumerate(ml) if n}
        if len(ds) == 1 and self.n_streams > 1:                # the usual case: one column slice and one split per output
            d = ds.pop()
            res = list(zip(*[o[:, :d].split(ml) for o in outs]))
            for s, n in enumerate(ml):                         # (a stream without rows keeps its own width)
                if n == 0 and self._joints[s] != d:
                    res[s] = tuple(o[:0, :self._joints[s]] for o in outs)
            return res
        res, at = [], 0
        for s, n in enumerate(ml):
            d = self._joints[s]
            res.append(tuple(o[at:at + n, :d] for o in outs))
            at += n
        return res

    # ------------------------------------------------------------------ staying in step with the source
    def _seen_now(self) -> np.ndarray:
        return np.array(self.decoder.n_seen, dtype=np.int64).reshape(-1).copy()

    def _check_in_step(self):
        if not np.array_equal(self._seen_now(), self._left):
            raise _lib.CpNativeError("the source was pushed or reset behind the stage (its n_seen is not what the stage left): the "
                                     "stage's rings no longer follow the streams; push and reset through the stage, or reset() it")

    def _check_models(self, has_rows):
        for s, rows in enumerate(has_rows):
            if rows and not self._joints[s]:
                raise _lib.CpNativeError(f"stream {s} has windows but no pose model: set_model or PoseFit.install first")

    # ------------------------------------------------------------------ API
    def apply(self, tail, cls=None):
        """The stage alone on tail inputs the caller already has (of the source's next windows, in order): tail (M, 512) in the
        decoder's compute dtype on the GPU and cls (M,) int32 (class ids, < 0: none) or None -> (raw, pose, angle); on a
        multi-stream source lists with one entry per stream (None: no windows) -> one such tuple per stream."""
        import torch
        tails = list(tail) if self.multi else [tail]
        clss = [None] * self.n_streams if cls is None else (list(cls) if self.multi else [cls])
        if len(tails) != self.n_streams or len(clss) != self.n_streams:
            raise ValueError(f"tail and cls must be sequences of {self.n_streams} entries (None or tensors)")
        dt = torch.float32 if self.decoder.dtype == "f32" else torch.bfloat16
        ms = []
        for s, (t, c) in enumerate(zip(tails, clss)):
            if t is None:
                ms.append(0)
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 2 or t.shape[1] != F or t.device.type != "cuda":
                raise ValueError(f"tail must be (M, 512) {self.decoder.dtype} tensors on the GPU")
            if c is not None and (not isinstance(c, torch.Tensor) or c.dtype != torch.int32 or tuple(c.shape) != (t.shape[0],)):
                raise ValueError("cls must be (M,) int32 tensors next to their tail inputs")
            ms.append(int(t.shape[0]))
        if cls is not None and any((c is None) != (t is None) for t, c in zip(tails, clss)):
            raise ValueError("tail and cls go together")
        self._check_models(ms)
        step = _lib.CP_ONLINE_MAX_WINDOWS
        outs = []
        for lo in range(0, max(max(ms), 1), step):
            m = np.array([min(max(n - lo, 0), step) for n in ms], dtype=np.int64)
            rows = int(m.sum())
            if rows == 0:
                continue
            row0 = np.zeros_like(m)
            np.cumsum(m[:-1], out=row0[1:])
            live = [s for s in range(self.n_streams) if m[s]]
            parts = [tails[s][lo:lo + int(m[s])] for s in live]
            t = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
            if t.data_ptr() % 16:
                t = t.clone()
            c = None
            if cls is not None:
                cp = [clss[s][lo:lo + int(m[s])] for s in live]
                c = (cp[0] if len(cp) == 1 else torch.cat(cp)).contiguous()
            outs.append(self._split(self._dev_push(t, F, c, row0, m, rows), m))
        self._left = self._seen_now()
        res = self._join(outs)
        return res if self.multi else res[0]

    def _join(self, outs):
        """per-launch per-stream (raw, pose, angle) -> per stream"""
        import torch
        if len(outs) == 1:
            return outs[0]
        res = []
        for s in range(self.n_streams):
            d = self._joints[s]
            if not outs:
                res.append((torch.empty(0, d, dtype=torch.float32, device=self.device), torch.empty(0, d, dtype=torch.int32, device=self.device),
                            torch.empty(0, d, dtype=torch.float32, device=self.device)))
            else:
                res.append(tuple(torch.cat([o[s][i] for o in outs]) for i in range(3)))
        return res

    def _behind(self, res_per_stream, row0: np.ndarray, m: np.ndarray):
        """the stage over the chain of launches the source just ran: its tail inputs are rows row0[s] .. of `tail_view()`"""
        import torch
        rows = int(m.sum())
        if rows == 0:
            return self._split(tuple(torch.empty(0, MAX_JOINTS, dtype=dt, device=self.device)
                                     for dt in (torch.float32, torch.int32, torch.float32)), m)
        c = None
        if self.gate is not None:                              # the gate's command of every row, packed in stream order
            from .online import _packed_rows
            cv = [r[-4].unsqueeze(1) if n else None for r, n in zip(res_per_stream, m.tolist())]
            c, ldc = _packed_rows(cv, row0, True, 1)           # (the gate's own packed output, as it lies)
            if ldc != 1:
                c = torch.cat([v for v in cv if v is not None])
        if self._tail is None:                                 # (the decoder's workspace tensor is allocated once)
            self._tail = self.decoder.tail_view()
        return self._split(self._dev_push(self._tail, F, c, row0, m, rows), m)

    def push(self, raw, return_logits: bool = False, return_windows: bool = False):
        """What the source's `push` takes (raw (n, 12), or one chunk per stream) -> the source's tuple(s) extended by raw, pose,
        angle: behind a gate (pred, voted[, logits][, windows], command, accepted, conf, margin, raw, pose, angle)."""
        import torch
        from .online import _check_raw
        self._check_in_step()
        kw = dict(return_logits=return_logits, return_windows=return_windows)
        if not self.multi:
            _check_raw(raw)
            self._check_models([True])
            step = STRIDE * self.decoder.max_windows
            parts = []
            for lo in range(0, max(int(raw.shape[0]), 1), step):
                res = self.source.push(raw[lo:lo + step], **kw)
                m = np.array([int(res[0].shape[0])], dtype=np.int64)
                parts.append(tuple(res) + self._behind([res], np.zeros(1, dtype=np.int64), m)[0])
            self._left = self._seen_now()
            return parts[0] if len(parts) == 1 else tuple(torch.cat([p[i] for p in parts]) for i in range(len(parts[0])))
        if isinstance(raw, torch.Tensor) or len(raw) != self.n_streams:
            raise ValueError(f"chunks must be a sequence of {self.n_streams} entries (None or (n, 12) tensors)")
        counts, live = [], []
        for c in raw:
            if c is not None:
                _check_raw(c, "each chunk")
            counts.append(0 if c is None else int(c.shape[0]))
            if counts[-1]:
                live.append(c)
        packed = torch.cat(live) if len(live) > 1 else (live[0].contiguous() if live else
                                                         torch.empty(0, 12, dtype=torch.float32, device=self.device))
        return self._push_packed(packed, np.asarray(counts, dtype=np.int64), kw)

    def push_packed(self, raw, counts, return_logits: bool = False, return_windows: bool = False):
        """`push` for samples packed in stream order, as the multi-stream decoders' `push_packed`."""
        from .online import _check_raw
        if not self.multi:
            raise TypeError("push_packed belongs to the multi-stream decoders")
        self._check_in_step()
        _check_raw(raw)
        cnt = np.asarray(counts, dtype=np.int64).reshape(-1)
        if cnt.shape[0] != self.n_streams or (cnt < 0).any() or int(cnt.sum()) != raw.shape[0]:
            raise ValueError(f"counts must hold {self.n_streams} entries >= 0 that sum to the samples of raw")
        return self._push_packed(raw.contiguous(), cnt, dict(return_logits=return_logits, return_windows=return_windows))

    def _push_packed(self, raw, counts: np.ndarray, kw: dict):
        import torch
        from .online import packed_rows, plan_push
        dec = self.decoder
        self._check_models((counts > 0).tolist())
        seen = np.array(dec.n_seen, dtype=np.int64)
        row0, m = packed_rows(seen, counts, dec.phase)
        if m.max() <= dec.max_windows and m.sum() <= dec.max_rows:
            rounds = [(counts, raw)]                           # the usual case: one chain of launches
        else:
            start = np.zeros_like(counts)
            np.cumsum(counts[:-1], out=start[1:])
            done = np.zeros_like(counts)
            rounds = []
            for take in plan_push(seen, counts, dec.phase, dec.max_windows, dec.max_rows):
                rounds.append((take, torch.cat([raw[start[s] + done[s]:start[s] + done[s] + take[s]] for s in np.nonzero(take)[0]])))
                done += take
        outs = []
        for take, piece in rounds:
            row0, m = packed_rows(seen, take, dec.phase)
            res = self.source.push_packed(piece, take, **kw)
            posed = self._behind(res, np.asarray(row0, dtype=np.int64), np.asarray(m, dtype=np.int64))
            outs.append([tuple(r) + p for r, p in zip(res, posed)])
            seen = seen + take
        self._left = self._seen_now()
        if len(outs) == 1:
            return outs[0]
        return [tuple(torch.cat([o[s][i] for o in outs]) for i in range(len(outs[0][s]))) for s in range(self.n_streams)]

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back (this waits for the device; a test and debugging aid): joints
        (0: no model), out (D,) the pose, and ring (entries, D), the q values from the oldest to the newest.  The layout is that
        of OknState (csrc/online_kinematics.cuh): int32 D, head, len, 5 unused, out[32], sum[32], rest[32], f32 lo[32], span[32],
        b[32], int32 ring[64][32], f32 W[32][512]."""
        import torch
        s = self._index(stream)
        if self.ws is None:
            return dict(joints=0, out=np.zeros(0, dtype=np.int64), ring=np.zeros((0, 0), dtype=np.int64))
        w = self.ws[:self.n_streams * _STATE_WORDS * 4].view(torch.int32).reshape(self.n_streams, _STATE_WORDS)[s]
        w = w[:_STATE_HEAD + 6 * MAX_JOINTS + MAX_SMOOTH * MAX_JOINTS].cpu().numpy()
        d, head, n = int(w[0]), int(w[1]), int(w[2])
        ring = w[_STATE_HEAD + 6 * MAX_JOINTS:].reshape(MAX_SMOOTH, MAX_JOINTS)
        at = [(head - n + i) % self.smooth for i in range(n)]
        return dict(joints=d, out=w[_STATE_HEAD:_STATE_HEAD + d].astype(np.int64), ring=ring[at][:, :d].astype(np.int64).reshape(n, d))

    def reset(self, streams=None):
        """Reset the source (a gate resets its decoder) and the stage (rings empty, pose 0; the models stay); on a multi-stream
        source the listed streams, default all."""
        if self.multi and streams is not None:
            idx = sorted({self._index(s) for s in streams})
            self.source.reset(idx)
            for s in idx:
                self._dev_reset(s)
        else:
            self.source.reset()
            self._dev_reset(-1)
        self._left = self._seen_now()
