"""Joint-angle decoding without a GPU (contrastiveprosthetics_amd/kinematics.py, include/cpnative.h cp_online_tail_offset and
cp_online_kin_*): the numpy definitions against loops and numpy.linalg.lstsq, the properties the definitions promise, and the
binding and host checks of the C entries."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from contrastiveprosthetics_amd import kinematics as K
from contrastiveprosthetics_amd import readout as R
from contrastiveprosthetics_amd.constants import WINDOW_EDGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG, ERR_WORKSPACE = 10001, 10002
F = np.float32
ENTRIES = ["cp_online_kin_moments", "cp_online_kin_apply", "cp_online_kin_score", "cp_online_kin_set_model", "cp_online_kin_reset",
           "cp_online_kin_push"]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def small_case(n, d, seed=0, n_groups=3):
    """n windows of rectified tail inputs, joint angles in 0..90 and n_groups groups, with unused windows (group -1) among them"""
    rng = np.random.default_rng(seed)
    u = np.maximum(rng.standard_normal((n, 512)) + 0.2, 0.0).astype(F)
    y = rng.uniform(0.0, 90.0, size=(n, d)).astype(F)
    groups = rng.integers(0, n_groups, size=n)
    groups[rng.random(n) < 0.15] = -1
    return u, y, groups.astype(np.int64)


PLANS = [((0, 1, 2), 1e-2), ((0, 2), 1.0)]


@pytest.fixture(scope="module")
def case100():
    u, y, groups = small_case(100, 17, seed=1)
    fit = K.fit_reference(u, y, PLANS, groups=groups, n_groups=3)
    for v in (u, y, groups, *[fit[key] for key in ("W", "b", "X", "G", "C", "weights")]):
        v.setflags(write=False)
    return u, y, groups, fit


# ---------------------------------------------------------------------------------------------------------------------------
# targets
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 19])
@pytest.mark.parametrize("lag", [0, 3])
def test_window_targets_against_a_loop(phase, lag):
    rng = np.random.default_rng(2)
    for n_samples in (0, 10, 11 + phase, 30 + phase, 211, 1000):
        glove = rng.standard_normal((n_samples, 5)).astype(F)
        m = max(0, (n_samples - phase - 2 * WINDOW_EDGE - 1 + 20) // 20)          # the windows of the recording
        want = []
        for k in range(m):
            at = phase + 20 * (k + lag) + WINDOW_EDGE
            if at >= n_samples:                                # off the end: this window and every later one is unused
                break
            want.append(glove[at])
        y = K.window_targets(glove, phase, lag)
        assert y.shape == (len(want), 5) and y.dtype == F
        assert same_bits(y, np.array(want, dtype=F).reshape(len(want), 5))
        assert max(0, m - lag) <= y.shape[0] <= m              # at most the last `lag` windows have no target
    glove = np.zeros((200, 2), dtype=F)
    glove[phase + 20 * lag + WINDOW_EDGE + 20, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        K.window_targets(glove, phase, lag)
    for bad in (np.zeros((10, 33), F), np.zeros((10, 0), F), np.zeros(10, F), np.zeros((10, 2))):
        with pytest.raises(ValueError, match="glove"):
            K.window_targets(bad)
    with pytest.raises(ValueError, match="lag"):
        K.window_targets(np.zeros((10, 2), F), 0, -1)
    with pytest.raises(ValueError, match="phase"):
        K.window_targets(np.zeros((10, 2), F), 20)


# ---------------------------------------------------------------------------------------------------------------------------
# moments and solve
# ---------------------------------------------------------------------------------------------------------------------------
def test_moments_are_the_readouts_with_the_windows_own_row(case100):
    """G is `readout.moments_reference`'s with every used window in one slot; an element of C is a scalar loop in window order"""
    u, y, groups, fit = case100
    w = fit["weights"]
    assert same_bits(w, K.uniform_weights(groups, 100)) and w[groups < 0].sum() == 0 and w[groups >= 0][0] == 1.0 / (groups >= 0).sum()
    G0, _ = R.moments_reference(u, np.zeros(100, dtype=np.int64), w, np.zeros((1, 16), F), groups, 3)
    assert same_bits(G0, fit["G"]) and same_bits(fit["G"], np.transpose(fit["G"], (0, 2, 1)))
    assert fit["C"].shape == (3, 513, 17)
    for r, a, d in ((1, 37, 5), (0, 512, 16), (2, 0, 0)):
        c = np.float64(0.0)
        for i in np.nonzero(groups == r)[0]:
            xa = np.float64(u[i, a]) if a < 512 else np.float64(1.0)
            c = c + w[i] * (xa * np.float64(y[i, d]))
        assert c == fit["C"][r, a, d]
    blocks = K.column_blocks(fit["C"])
    assert blocks.shape == (2, 3, 513, 16) and same_bits(blocks[0], fit["C"][:, :, :16]) and same_bits(blocks[1, :, :, 0], fit["C"][:, :, 16])
    assert not blocks[1, :, :, 1:].any()


def test_fit_reference_against_lstsq_by_the_normal_equation_residual(case100):
    """The weighted ridge problem as numpy.linalg.lstsq solves it (rows sqrt(w_i) x_i, then sqrt(ridge) e_a for the penalised
    coordinates), compared by the normal-equation residual |A X - B|_inf of the float64 solution.  The bound is the one
    tests/test_online_readout_host.py derives: a Cholesky solve is backward stable with |dA| <= g(3n+1) |L||L^T| (Higham,
    Accuracy and Stability, th. 10.4) and | |L||L^T| |_inf <= n |A|_inf, so the residual stays within
    (3n+1) n u |A|_inf |X|_inf; the sequential moments differ from the BLAS ones by at most (N + 2) u per element relative to
    sums of absolute values (all terms are >= 0 here: u is rectified and the angles are >= 0), which adds
    (N + 2) u (|A|_inf |X|_inf + |B|_inf); n = 513, u = 2^-53."""
    u, y, groups, fit = case100
    n_w, n, eps = u.shape[0], 513, 2.0 ** -53
    assert (u >= 0).all() and (y >= 0).all()
    xm = np.concatenate([u.astype(np.float64), np.ones((n_w, 1))], axis=1)
    w = fit["weights"]
    for t, (grp, lam) in enumerate(PLANS):
        wt = np.where(np.isin(groups, grp), w, 0.0)
        a = xm.T @ (wt[:, None] * xm) + lam * np.diag(np.r_[np.ones(512), 0.0])
        b = xm.T @ (wt[:, None] * y.astype(np.float64))
        assert fit["status"][t] == 0
        x = fit["X"][t]
        assert x.shape == (513, 17)
        a_inf, x_inf, b_inf = np.abs(a).sum(axis=1).max(), np.abs(x).sum(axis=1).max(), np.abs(b).sum(axis=1).max()
        bound = ((3 * n + 1) * n * a_inf * x_inf + (n_w + 2) * (a_inf * x_inf + b_inf)) * eps
        res = np.abs(a @ x - b).sum(axis=1).max()
        rows = np.concatenate([np.sqrt(wt)[:, None] * xm, np.sqrt(lam) * np.eye(513)[:512]])
        rhs = np.concatenate([np.sqrt(wt)[:, None] * y.astype(np.float64), np.zeros((512, 17))])
        x_ls = np.linalg.lstsq(rows, rhs, rcond=None)[0]
        ls_res = np.abs(a @ x_ls - b).sum(axis=1).max()
        print(f"plan {t}: residual {res:.3e}, numpy.linalg.lstsq {ls_res:.3e}, bound {bound:.3e}, |X - X_lstsq| {np.abs(x - x_ls).max():.3e}")
        assert res <= bound, (t, res, bound)
        assert same_bits(fit["W"][t], x[:512].T.astype(F)) and same_bits(fit["b"][t], x[512].astype(F))
        wrong = x.copy()
        wrong[7] *= 1.0 + 1e-4                                 # (an a-priori bound: it tells a row that is off in the fourth digit)
        assert np.abs(a @ wrong - b).sum(axis=1).max() > bound


def test_column_blocks_at_16_and_17_joints_give_the_same_first_16(case100):
    u, y, groups, fit = case100
    fit16 = K.fit_reference(u, np.ascontiguousarray(y[:, :16]), PLANS, groups=groups, n_groups=3)
    assert fit16["W"].shape == (2, 16, 512) and fit["W"].shape == (2, 17, 512)
    assert same_bits(fit16["W"], np.ascontiguousarray(fit["W"][:, :16])) and same_bits(fit16["b"], np.ascontiguousarray(fit["b"][:, :16]))
    assert same_bits(fit16["G"], fit["G"]) and fit16["status"].tolist() == fit["status"].tolist() == [0, 0]
    # a zero right-hand side solves to zero: the padding of the last block never leaks
    zero = K.solve_reference(fit["G"], np.zeros((3, 513, 3)), PLANS)
    assert not zero[0].any() and not zero[1].any() and zero[2].tolist() == [0, 0]


def test_the_plan_that_fails_gives_status_1_and_zeros():
    u = np.zeros((20, 512), dtype=F)
    y = np.tile(np.array([[10.0, 30.0, 50.0]], dtype=F), (20, 1))
    fit = K.fit_reference(u, y, ridge=[0.0, 0.5])
    assert fit["status"].tolist() == [1, 0]
    assert not fit["W"][0].any() and not fit["b"][0].any() and fit["W"].shape == (2, 3, 512)
    assert not fit["W"][1].any() and np.allclose(fit["b"][1], [10.0, 30.0, 50.0], atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
# the pose matvec, the state machine and the score
# ---------------------------------------------------------------------------------------------------------------------------
def test_pose_reference_is_the_scalar_loop_of_the_docstring():
    rng = np.random.default_rng(3)
    u = np.maximum(rng.standard_normal((3, 512)), 0).astype(F)
    W, b = (0.05 * rng.standard_normal((4, 512))).astype(F), rng.standard_normal(4).astype(F)
    a = K.pose_reference(u, W, b)
    assert a.shape == (3, 4) and a.dtype == F
    for i in range(3):
        for d in range(4):
            p = [F(0.0)] * 64
            for lane in range(64):
                for j in range(8):
                    p[lane] = F(p[lane] + F(W[d, lane + 64 * j] * u[i, lane + 64 * j]))
            s = 32
            while s:
                for lane in range(s):
                    p[lane] = F(p[lane] + p[lane + s])
                s //= 2
            assert F(p[0] + b[d]).tobytes() == a[i, d].tobytes(), (i, d)
    assert np.abs(a - (u.astype(np.float64) @ W.astype(np.float64).T + b)).max() < 1e-4
    assert same_bits(K.pose_reference(R.round_bf16(u).astype(F), W, b), K.pose_reference(R.round_bf16(u), W, b).astype(F))


def crafted_rows():
    """Three joints that read u[0], u[1], u[2] (W is a selection, so a = u + b exactly), lo 0 and span 1: rows that clamp low
    and high, a NaN row, rows with the class "none", and steps large enough to be rate-limited both ways"""
    W = np.zeros((3, 512), dtype=F)
    W[0, 0] = W[1, 1] = W[2, 2] = 1.0
    b = np.array([0.0, 0.125, -0.125], dtype=F)
    vals = [0.1, 0.1, 0.9, 0.95, 1.5, 1.7, 0.9, -0.5, -0.2, 0.05, np.nan, 0.5, 0.5, 0.5, 0.52, 0.3, 0.31, 0.8, 0.8, 0.8, 0.8, 0.0, 0.0,
            0.0, 0.0, 0.0, 0.6, 0.61, 0.62, 0.63, 0.64, 0.65, 0.66]
    u = np.zeros((len(vals), 512), dtype=F)
    u[:, 0] = vals
    u[:, 1] = np.roll(np.nan_to_num(np.array(vals, dtype=F), nan=0.4), 3)
    u[:, 2] = 1.0 - np.nan_to_num(np.array(vals, dtype=F), nan=0.2)
    u[:, 3:] = 0.25                                            # (times W = 0: nothing)
    cls = np.full(len(vals), 4, dtype=np.int64)
    cls[[12, 13, 24]] = -1
    lo, span, rest = np.zeros(3, F), np.ones(3, F), np.array([100, 2000, 4096], dtype=np.int32)
    return W, b, lo, span, rest, u, cls


EVENTS = {"nan", "clamp_low", "clamp_high", "none", "ring_filling", "rise_limited", "fall_limited"}


def test_joint_reference_gives_the_same_rows_for_any_cut():
    W, b, lo, span, rest, u, cls = crafted_rows()
    whole = K.JointReference(W, b, lo, span, rest, smooth=4, rate=600)
    raw, pose, angle = whole.push(u, cls)
    assert whole.events == EVENTS, whole.events                # every event is reached before anything is compared
    assert raw.dtype == F and pose.dtype == np.int32 and angle.dtype == F and raw.shape == pose.shape == angle.shape == (len(u), 3)
    assert (pose >= 0).all() and (pose <= K.ONE).all() and (np.abs(np.diff(pose, axis=0)) <= 600).all() and np.abs(pose[0]).max() <= 600
    assert same_bits(angle, (pose.astype(F) / F(4096)) * span + lo)
    for cuts in ([1] * len(u), [16, 17], [5, 0, 7, 21], [25, 8]):
        ref = K.JointReference(W, b, lo, span, rest, smooth=4, rate=600)
        parts, at = [], 0
        for n in cuts:
            parts.append(ref.push(u[at:at + n], cls[at:at + n]))
            at += n
        assert at == len(u)
        for i, want in enumerate((raw, pose, angle)):
            assert same_bits(np.concatenate([p[i] for p in parts]), want), (cuts, i)
        st, st0 = ref.state(), whole.state()
        assert same_bits(st["out"], st0["out"]) and same_bits(st["ring"], st0["ring"]) and st["ring"].shape == (4, 3)
    # a scalar walk of joint 0 without a class input
    ref = K.JointReference(W, b, lo, span, rest, smooth=4, rate=600)
    _, pose0, _ = ref.push(u)
    ring, out = [], 0
    for i, v in enumerate(u[:, 0].tolist()):
        q = 100 if np.isnan(v) else int(np.rint(F(min(max(F(v), F(0)), F(1))) * F(4096)))
        ring = (ring + [q])[-4:]
        s = sum(ring) // len(ring)
        out = min(out + 600, s) if s > out else max(out - 600, s)
        assert pose0[i, 0] == out, i
    ref.reset()
    assert same_bits(ref.push(u)[1], pose0)


def test_without_smoothing_and_rate_limit_the_pose_is_q():
    W, b, lo, span, rest, u, cls = crafted_rows()
    ref = K.JointReference(W, b, lo, span, rest, smooth=1, rate=K.ONE)
    raw, pose, angle = ref.push(u)
    assert same_bits(pose.astype(np.int64), ref.q)
    t = (raw - lo) / span
    want = np.where(np.isnan(t), rest, np.rint(np.clip(np.nan_to_num(t), 0, 1) * F(4096)).astype(np.int64))
    assert same_bits(pose.astype(np.int64), want.astype(np.int64))
    assert {"nan", "clamp_low", "clamp_high"} <= ref.events and "rise_limited" not in ref.events and "none" not in ref.events
    assert (ref.push(u, np.full(len(u), -1))[1] == rest).all()         # the class "none" throughout: the resting pose


def test_score_reference_against_a_loop_and_the_metrics():
    rng = np.random.default_rng(5)
    y = rng.uniform(0, 90, size=(60, 4)).astype(F)
    pred = (y[None] + rng.standard_normal((3, 60, 4))).astype(F)
    groups = rng.integers(-1, 3, size=60)
    masks = [0b001, 0b110, 0]
    sums = K.score_reference(pred, y, groups, masks)
    assert sums.shape == (3, 4, 7) and not sums[2].any()
    for p, mask in enumerate(masks[:2]):
        for d in (0, 3):
            s = [np.float64(0.0)] * 7
            for i in range(60):
                if groups[i] < 0 or not (mask >> groups[i]) & 1:
                    continue
                yy, q = np.float64(y[i, d]), np.float64(pred[p, i, d])
                e = q - yy
                for j, v in enumerate((np.float64(1.0), yy, yy * yy, q, q * q, yy * q, e * e)):
                    s[j] = s[j] + v
            assert same_bits(np.array(s), sums[p, d]), (p, d)
    m = K.metrics(sums)
    sel = np.isin(groups, [1, 2])
    e = pred[1][sel].astype(np.float64) - y[sel].astype(np.float64)
    assert np.allclose(m["rmse"][1], np.sqrt((e * e).mean(axis=0)), rtol=1e-12)
    assert np.allclose(m["r"][1], [np.corrcoef(pred[1][sel][:, d], y[sel][:, d])[0, 1] for d in range(4)], rtol=1e-9)
    assert np.allclose(m["r2"][1], 1 - (e * e).sum(axis=0) / ((y[sel] - y[sel].mean(axis=0)) ** 2).sum(axis=0), rtol=1e-9)
    assert np.isnan(m["rmse"][2]).all() and np.isnan(m["rmse_mean"][2]) and np.isclose(m["rmse_mean"][0], m["rmse"][0].mean())


def test_the_tie_rule_of_the_pick_and_the_synthetic_person():
    lam = np.array([0.01, 0.1, 1.0])
    sums = np.zeros((1, 2, 3, 2, 7))
    sums[..., 0] = 10.0
    sums[..., 6] = [[[4.0, 4.0], [1.0, 1.0], [1.0, 1.0]]] * 2
    out = K._pick_tables(sums, np.zeros((1, 2, 3), dtype=np.int32), lam, [0], 2)
    assert out["best"] == (0, 2) and out["ridge"] == 1.0 and out["lag"] == 0 and out["sums"][0, 0, 0, 6] == 8.0
    status = np.zeros((1, 2, 3), dtype=np.int32)
    status[0, 1, 2] = 5
    out = K._pick_tables(sums, status, lam, [0], 2)
    assert out["best"] == (0, 1) and not out["ok"][0, 2]
    # the synthetic person: the tail inputs lead the angles by `delay` windows, and a held-out fit finds that lag
    p = K.kinematics_recording(k=4, reps=3, segment=12, joints=3, delay=2, seed=0)
    assert p["u"].shape == (144, 512) and (p["u"] >= 0).all() and p["glove"].shape == (p["n_samples"], 3)
    assert same_bits(K.window_targets(p["glove"]), p["y"])
    out = K.pick_pose_reference(p["u"], p["glove"], (p["rep"], p["n_rep"]), ridges=[1e-2], lags=(0, 2))
    print("mean held-out RMSE per lag:", out["rmse_mean"][:, 0])
    assert out["best"] == (1, 0) and out["lag"] == 2 and out["rmse_mean"][1, 0] < out["rmse_mean"][0, 0]


def test_the_python_layer_refuses_bad_arguments():
    u, y, groups = small_case(20, 3, seed=6)
    with pytest.raises(ValueError, match="512"):
        K.moments_reference(u[:, :100], y)
    with pytest.raises(ValueError, match="targets"):
        K.moments_reference(u, y[:5])
    with pytest.raises(ValueError, match="targets"):
        K.moments_reference(u, np.zeros((20, 33), F))
    bad = y.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        K.moments_reference(u, bad)
    with pytest.raises(ValueError, match="number of groups"):
        K.moments_reference(u, y, None, groups, n_groups=17)
    with pytest.raises(ValueError, match="weights"):
        K.moments_reference(u, y, np.ones(5))
    W, b = np.zeros((3, 512), F), np.zeros(3, F)
    for kw, what in ((dict(span=[1, 0, 1]), "span"), (dict(span=[1, np.inf, 1]), "span"), (dict(lo=[0, np.nan, 0]), "lo"),
                     (dict(rest=[0, 4097, 0]), "rest"), (dict(rest=[0.5, 1, 2]), "rest"), (dict(smooth=0), "smooth"),
                     (dict(smooth=65), "smooth"), (dict(rate=0), "rate"), (dict(rate=4097), "rate")):
        args = dict(lo=[0, 0, 0], span=[1, 1, 1], rest=[0, 0, 0], smooth=5, rate=100)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            K.JointReference(W, b, **args)
    with pytest.raises(ValueError, match="W"):
        K.JointReference(np.zeros((33, 512), F), np.zeros(33, F), np.zeros(33), np.ones(33), np.zeros(33, dtype=int))
    fit = K.PoseFit(np.zeros((2, 3, 512), F), np.zeros((2, 3), F), [0, 7], [((0,), 0.1), ((0,), 0.0)], {0: 30}, [0] * 3, [1] * 3, [0] * 3)

    class Stage:
        multi, got = False, None

        def set_model(self, *a):
            self.got = a

    st = Stage()
    with pytest.raises(ValueError, match="positive definite"):
        fit.install(st, 1)
    with pytest.raises(IndexError):
        fit.install(st, 2)
    with pytest.raises(ValueError, match="stream="):
        fit.install(st, 0, stream=1)
    assert st.got is None
    fit.install(st, 0)
    assert st.got[0].shape == (3, 512) and len(st.got) == 5
    lo, span, rest = K.limits(y, np.arange(20) % 2, rest_class=1)
    assert (span > 0).all() and lo.dtype == span.dtype == F and rest.dtype == np.int32 and (rest >= 0).all() and (rest <= K.ONE).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the binding and the host checks of the entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_constants_and_symbols_match_the_header(lib):
    from contrastiveprosthetics_amd import _lib
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in ENTRIES:
        assert hasattr(raw, n) and n in _lib.SYMBOLS, n
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert m and len(m.group(1).split(",")) == len(_lib.SYMBOLS[n][1]), n
    for n in ("cp_online_tail_offset", "cp_online_kin_workspace_bytes"):
        assert hasattr(raw, n) and n in _lib.SYMBOLS and re.search(r"\bsize_t\s+%s\s*\(" % n, hdr), n
    for name in ("CP_ONLINE_KIN_MAX_JOINTS", "CP_ONLINE_KIN_MAX_SMOOTH", "CP_ONLINE_KIN_ONE", "CP_ONLINE_KIN_SUMS"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(_lib, name), name
    assert (K.MAX_JOINTS, K.MAX_SMOOTH, K.ONE, K.SUMS, K.BLOCKS) == (32, 64, 4096, 7, 2)
    body = hdr[hdr.index("typedef struct cp_online_kin_config {"):hdr.index("} cp_online_kin_config;")]
    assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in _lib.cp_online_kin_config._fields_]
    a256 = lambda n: (n + 255) // 256 * 256
    assert lib.cp_online_kin_workspace_bytes(0) == lib.cp_online_kin_workspace_bytes(1) == a256(4 * K._STATE_WORDS)
    assert lib.cp_online_kin_workspace_bytes(256) == a256(256 * 4 * K._STATE_WORDS) and K._STATE_WORDS == 18632


def test_tail_offset_is_the_last_block_of_the_pinned_totals(lib):
    """H1, the tail inputs, is the last block `ol_carve` takes: the offset is the form's pinned total
    (tests/test_online_workspace_host.py) minus the block, rows rounded up to 16, 512 values each, 256-aligned"""
    from contrastiveprosthetics_amd import _lib
    a256 = lambda n: (n + 255) // 256 * 256
    totals = {(0, 0): ([8055296, 8055296, 8137984, 9295616], [4041216, 4041216, 4082944, 4667136]),
              (1, 0): ([8359936, 8359936, 8639232, 12549376], [4272128, 4272128, 4436736, 6741248]),
              (0, 1): ([8055552, 8153600, 8597760, 31101184, 348623104], [4041472, 4098560, 4337920, 16642304, 176877824]),
              (1, 1): ([8360192, 8802304, 10524416, 100345344, 1172841984], [4272384, 4599808, 5748480, 67012096, 699106816])}
    pairs = [(1, 1), (3, 17), (7, 100), (256, 4096), (256, 65536)]
    for (adaptive, multi), per_dtype in totals.items():
        for dt, want in zip((_lib.CP_F32, _lib.CP_BF16), per_dtype):
            es = 4 if dt == _lib.CP_F32 else 2
            cfg = _lib.cp_online_config()
            cfg.dtype, cfg.vote, cfg.n_coef = dt, 25, 2
            shapes = pairs if multi else [(1, m) for m in (1, 16, 17, 256)]
            for (s, rows), total in zip(shapes, want):
                cfg.max_windows = min(rows, 256)
                off = lib.cp_online_tail_offset(ctypes.byref(cfg), s, rows, adaptive, multi)
                assert off == total - a256((rows + 15) // 16 * 16 * 512 * es), (adaptive, multi, dt, s, rows)
                assert off % 256 == 0
    cfg = _lib.cp_online_config()
    cfg.dtype, cfg.max_windows = 0, 16
    for bad, what in ((dict(dtype=2), "dtype"), (dict(max_windows=0), "max_windows"), (dict(max_windows=257), "max_windows")):
        c2 = _lib.cp_online_config()
        c2.dtype, c2.max_windows = bad.get("dtype", 0), bad.get("max_windows", 16)
        assert lib.cp_online_tail_offset(ctypes.byref(c2), 1, 16, 0, 0) == 0
        assert b"cp_online_tail_offset" in lib.cp_last_error() and what.encode() in lib.cp_last_error()
    for args, what in (((0, 16, 0, 1), "n_streams"), ((257, 16, 0, 1), "n_streams"), ((2, 0, 1, 1), "max_rows"), ((2, 65537, 1, 1), "max_rows"),
                       ((2, 16, 0, 0), "one stream")):
        assert lib.cp_online_tail_offset(ctypes.byref(cfg), *args) == 0 and what.encode() in lib.cp_last_error()
    assert lib.cp_online_tail_offset(None, 1, 16, 0, 0) == 0 and b"config" in lib.cp_last_error()


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory for every pointer: each refusal returns before a launch, which on a machine without a GPU would fail otherwise"""
    from contrastiveprosthetics_amd import _lib
    buf = ctypes.create_string_buffer(1 << 20)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 40

    def err(rc, entry, what, code=ERR_ARG):
        assert rc == code, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    name = "cp_online_kin_moments"
    mo = lambda u=p, dtype=0, n=8, group=p, w=p, y=p, ldy=20, d=20, r=2, G=p, Cm=p, sc=p, nb=big: \
        lib.cp_online_kin_moments(u, dtype, n, group, w, y, ldy, d, r, G, Cm, sc, nb, None)
    err(mo(dtype=2), name, "dtype")
    for n in (-1, (1 << 24) + 1):
        err(mo(n=n), name, "n_rows")
    for d in (0, 33):
        err(mo(d=d, ldy=40), name, "n_joints")
    for r in (0, 17):
        err(mo(r=r), name, "n_groups")
    err(mo(ldy=19), name, "ldy")
    for arg in ("u", "group", "w", "y", "G", "Cm", "sc"):
        err(mo(**{arg: None}), name, "required")
    for arg in ("u", "group", "w", "y", "G", "Cm", "sc"):
        err(mo(**{arg: p + 2}), name, "misaligned")
    err(mo(w=p + 4), name, "misaligned")
    err(mo(u=p + 8), name, "misaligned")
    err(mo(nb=256), name, "scratch too small", ERR_WORKSPACE)

    name = "cp_online_kin_apply"
    ap = lambda u=p, dtype=1, n=8, W=p, b=p, P=2, d=20, out=p: lib.cp_online_kin_apply(u, dtype, n, W, b, P, d, out, None)
    err(ap(dtype=-1), name, "dtype")
    for n in (-1, (1 << 24) + 1):
        err(ap(n=n), name, "n_rows")
    for P in (-1, 257):
        err(ap(P=P), name, "n_plans")
    for d in (0, 33):
        err(ap(d=d), name, "n_joints")
    assert ap(n=0) == 0 and ap(P=0) == 0 and ap(n=0, u=None) == 0
    for arg in ("u", "W", "b", "out"):
        err(ap(**{arg: None}), name, "required")
    for arg in ("u", "W", "b", "out"):
        err(ap(**{arg: p + 2}), name, "misaligned")
    err(ap(W=p + 4), name, "misaligned")

    name = "cp_online_kin_score"
    masks = (ctypes.c_uint32 * 4)(1, 2, 4, 3)
    sc = lambda pred=p, y=p, ldy=20, group=p, masks=masks, P=4, n=8, d=20, sums=p: \
        lib.cp_online_kin_score(pred, y, ldy, group, masks, P, n, d, sums, None)
    for n in (-1, (1 << 24) + 1):
        err(sc(n=n), name, "n_rows")
    for P in (-1, 257):
        err(sc(P=P), name, "n_plans")
    for d in (0, 33):
        err(sc(d=d, ldy=40), name, "n_joints")
    err(sc(ldy=19), name, "ldy")
    assert sc(P=0) == 0
    for arg in ("pred", "y", "group", "masks", "sums"):
        err(sc(**{arg: None}), name, "required")
    for arg in ("pred", "y", "group", "sums"):
        err(sc(**{arg: p + 2}), name, "misaligned")
    err(sc(sums=p + 4), name, "misaligned")
    err(sc(masks=(ctypes.c_uint32 * 4)(1, 2, 1 << 16, 3)), name, "mask")

    cfg = _lib.cp_online_kin_config()
    cfg.smooth, cfg.rate = 5, 4096
    ws_bytes = lib.cp_online_kin_workspace_bytes(3)
    assert ws_bytes <= 1 << 19
    f3 = lambda *v: (ctypes.c_float * 20)(*(list(v) + [1.0] * (20 - len(v))))
    lo, span, rest = f3(0.0), f3(1.0), (ctypes.c_int32 * 20)(*([0] * 20))

    def entries(c=cfg, s=3, ws=p, nb=ws_bytes):
        """every stage entry with the same config, stream count and workspace"""
        cp = ctypes.byref(c) if c is not None else None
        return [("cp_online_kin_set_model", lib.cp_online_kin_set_model(cp, s, ws, nb, 0, p, p, 20, lo, span, rest, None)),
                ("cp_online_kin_reset", lib.cp_online_kin_reset(cp, s, ws, nb, -1, None)),
                ("cp_online_kin_push", lib.cp_online_kin_push(cp, s, ws, nb, p, 0, 512, None, p, p, 8, p, p, p, None))]

    def every(what, code=ERR_ARG, **kw):
        for name, rc in entries(**kw):
            assert rc == code, (name, what, rc)
        # (cp_last_error holds the last one's text; each entry's own name is checked below)

    every("config", c=None)
    every("workspace", ws=None)
    for s in (0, 257):
        every("n_streams", s=s)
    for smooth in (0, 65):
        c2 = _lib.cp_online_kin_config()
        c2.smooth, c2.rate = smooth, 100
        every("smooth", c=c2)
        assert b"cp_online_kin_push" in lib.cp_last_error() and b"smooth outside 1..64" in lib.cp_last_error()
    for rate in (0, 4097):
        c2 = _lib.cp_online_kin_config()
        c2.smooth, c2.rate = 5, rate
        every("rate", c=c2)
        assert b"rate outside 1..4096" in lib.cp_last_error()
    every("aligned", ws=p + 64)
    assert b"not 256-byte aligned" in lib.cp_last_error()
    every("too small", code=ERR_WORKSPACE, nb=ws_bytes - 256)      # a short workspace
    assert b"workspace too small" in lib.cp_last_error()

    name = "cp_online_kin_set_model"
    sm = lambda index=0, W=p, b=p, d=20, lo=lo, span=span, rest=rest: \
        lib.cp_online_kin_set_model(ctypes.byref(cfg), 3, p, ws_bytes, index, W, b, d, lo, span, rest, None)
    for index in (-1, 3):
        err(sm(index=index), name, "stream index")
    for d in (0, 33):
        err(sm(d=d), name, "n_joints outside 1..32")
    for arg in ("W", "b", "lo", "span", "rest"):
        err(sm(**{arg: None}), name, "required")
    err(sm(W=p + 4), name, "misaligned")
    err(sm(b=p + 2), name, "misaligned")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        err(sm(span=f3(1.0, bad)), name, "span")
    err(sm(lo=f3(0.0, float("inf"))), name, "lo")
    for bad in (-1, 4097):
        err(sm(rest=(ctypes.c_int32 * 20)(0, bad)), name, "rest")

    name = "cp_online_kin_reset"
    for index in (-2, 3):
        err(lib.cp_online_kin_reset(ctypes.byref(cfg), 3, p, ws_bytes, index, None), name, "stream index")

    name = "cp_online_kin_push"
    pu = lambda tail=p, dtype=0, ldt=512, cls=None, row0=p, m=p, rows=8, raw=p, pose=p, angle=p: \
        lib.cp_online_kin_push(ctypes.byref(cfg), 3, p, ws_bytes, tail, dtype, ldt, cls, row0, m, rows, raw, pose, angle, None)
    err(pu(dtype=2), name, "dtype")
    for rows in (-1, 65537):
        err(pu(rows=rows), name, "total_rows")
    assert pu(rows=0) == 0 and pu(rows=0, tail=None) == 0      # an empty call
    err(pu(ldt=511), name, "ldt")
    for arg in ("tail", "row0", "m", "raw", "pose", "angle"):
        err(pu(**{arg: None}), name, "required")
    for arg in ("tail", "cls", "row0", "m", "raw", "pose", "angle"):
        err(pu(**{arg: p + 2}), name, "misaligned")
    err(pu(tail=p + 8), name, "misaligned")
    err(pu(dtype=1, ldt=516), name, "misaligned")              # bf16 rows of 1032 bytes are not 16-byte aligned
