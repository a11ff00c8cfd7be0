"""The pose filter's definitions (contrastiveprosthetics_amd/kalman.py) on the host: the trajectory samples and moments against
loops, the design against an independent float64 version written with numpy.linalg, `FilterReference` for any cut of rows that
reach every event, the sweep against `FilterReference`, the synthetic person, the tie rule of the pick, and every refusal of the
Python layer and of the cp_online_kf_* entries (which return before any device call)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from contrastiveprosthetics_amd import kalman as KF
from contrastiveprosthetics_amd import kinematics as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG, ERR_WORKSPACE = 10001, 10002
F = np.float32
ENTRIES = ["cp_online_kf_moments", "cp_online_kf_design", "cp_online_kf_sweep", "cp_online_kf_set_model", "cp_online_kf_reset",
           "cp_online_kf_push"]
EVENTS = {"not_started", "start", "run", "hold", "none", "clamp_low", "clamp_high", "rise_limited", "fall_limited"}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_f32(got, want):
    """f32 arrays as bit patterns; where both hold a NaN its payload is not compared (the definition does not fix one)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != F or want.dtype != F:
        return False
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def filter_case(n, d, seed=0, n_groups=3):
    """n windows of d joint angles that move together through a smoothed random walk (five latent motions), a noisy readout of
    them, n_groups groups in blocks with one unused window inside a block, and the limits of a stage"""
    rng = np.random.default_rng(seed)
    latent = np.cumsum(rng.standard_normal((n + 8, 5)), axis=0)
    latent = np.stack([latent[i:i + n] for i in range(8)]).mean(axis=0)
    y = (45.0 + 6.0 * latent @ rng.standard_normal((5, d)) / np.sqrt(5.0) + 0.05 * rng.standard_normal((n, d))).astype(F)
    a = (y + 3.0 * rng.standard_normal((n, d))).astype(F)
    groups = np.minimum(np.arange(n) * n_groups // max(n, 1), n_groups - 1).astype(np.int64)
    if n >= 8:
        groups[n // 2 + 1] = -1                                # an unused window in the middle of a block
    lo, span, rest = K.limits(y, low=10.0, high=90.0)
    return a, y, groups, lo, span, rest


def test_centre_is_joint_angles_expression():
    lo, span, rest = np.array([1.5, -2.0], dtype=F), np.array([3.0, 7.0], dtype=F), np.array([1000, 4096], dtype=np.int32)
    c = KF.centre(lo, span, rest)
    want = [F(1.5) + (F(1000) / F(4096)) * F(3.0), F(-2.0) + (F(4096) / F(4096)) * F(7.0)]
    assert c.dtype == F and same_bits(c, np.array(want, dtype=F))


def test_trajectory_triples_against_a_loop_with_a_gap_and_a_group_change():
    a, y, _, lo, span, rest = filter_case(14, 3, seed=1)
    groups = np.array([0, 0, 0, 0, -1, 0, 0, 0, 1, 1, 1, 1, 2, 2])
    c = KF.centre(lo, span, rest)
    k, gk, s0, s1, e1 = KF.triples_reference(a, y, groups, 3, c)
    assert k.tolist() == [1, 2, 6, 9, 10] and gk.tolist() == [0, 0, 0, 1, 1]       # (group 2 has two windows: none counts)
    for i, kk in enumerate(k.tolist()):
        th = [[F(F(y[j, d]) - c[d]) for d in range(3)] for j in (kk - 1, kk, kk + 1)]
        want0 = th[1] + [F(th[1][d] - th[0][d]) for d in range(3)]
        want1 = th[2] + [F(th[2][d] - th[1][d]) for d in range(3)]
        assert same_bits(s0[i], np.array(want0, dtype=F)) and same_bits(s1[i], np.array(want1, dtype=F))
        assert same_bits(e1[i], np.array([F(a[kk + 1, d] - y[kk + 1, d]) for d in range(3)], dtype=F))
    mom = KF.moments_reference(a, y, groups, 3, c)
    assert mom["n"].tolist() == [3, 2, 0] and not mom["G"][2].any() and not mom["E"][2].any()
    G = np.zeros((6, 6))
    for i in (0, 1, 2):                                        # a scalar loop in window order
        for p in range(6):
            for q in range(6):
                G[p, q] = G[p, q] + float(s0[i][p]) * float(s0[i][q])
    assert same_bits(mom["G"][0], G)
    assert np.array_equal(mom["C"][1], sum(np.outer(s1[i].astype(np.float64), s0[i].astype(np.float64)) for i in (3, 4)))
    assert np.array_equal(mom["S"][1][0, 0], sum(float(s1[i][0]) ** 2 for i in (3, 4)))
    for n in (0, 1, 2):
        assert not KF.moments_reference(a[:n], y[:n], groups[:n], 3, c)["n"].any()


def design_linalg(mom, plans):
    """the design in float64 with numpy.linalg (an independent order of every sum), the same T iterations"""
    out = []
    for groups, lam, rho, kappa, T in plans:
        sel = list(groups)
        n = mom["n"][sel].sum()
        G, Cm, S, E = (mom[k][sel].sum(axis=0) / n for k in ("G", "C", "S", "E"))
        n2, d = G.shape[0], E.shape[0]
        A = np.linalg.solve(G + lam * np.trace(G) / n2 * np.eye(n2), Cm.T).T
        Rm = S - A @ Cm.T - Cm @ A.T + A @ G @ A.T
        W = rho * (0.5 * (Rm + Rm.T) + 1e-6 * np.trace(S) / n2 * np.eye(n2))
        Q = kappa * (E + 1e-6 * np.trace(E) / d * np.eye(d))
        H = np.eye(d, n2)
        P = W.copy()
        for _ in range(T):
            Pm = A @ P @ A.T + W
            Kg = np.linalg.solve(H @ Pm @ H.T + Q, H @ Pm).T
            J = np.eye(n2) - Kg @ H
            P = J @ Pm @ J.T + Kg @ Q @ Kg.T
            P = 0.5 * (P + P.T)
        out.append((J @ A, Kg, np.linalg.cond(G + lam * np.trace(G) / n2 * np.eye(n2)), np.linalg.cond(H @ Pm @ H.T + Q)))
    return out


# The bound of the comparison below.  A bound from condition estimates was looked at first: the backward error of the Cholesky
# solve behind A, (3 * 2D + 1) eps cond(G + lambda I) with cond = 4e2 .. 3e4 here, carried through 2D-term products, gives
# 1e-11 (D = 1) to 2e-8 (D = 17), four orders above what the recursion, which contracts errors, leaves.  The bound is therefore
# 100 x the largest difference measured on these fixed inputs, in max|.| of M and K before their rounding to f32, T = 64:
# D = 1: 2.3e-16, D = 3: 2.9e-15, D = 17: 1.4e-12 (DESIGN 7zh records them).
LINALG_BOUND = {1: 100 * 2.3e-16, 3: 100 * 2.9e-15, 17: 100 * 1.4e-12}


@pytest.mark.parametrize("d", [1, 3, 17])
def test_design_reference_against_numpy_linalg(d):
    a, y, groups, lo, span, rest = filter_case(240, d, seed=2 + d)
    mom = KF.moments_reference(a, y, groups, 3, KF.centre(lo, span, rest))
    plans = [((0, 1, 2), 1e-3, 1.0, 1.0, 64), ((0, 2), 1e-3, 0.25, 4.0, 64)]
    des = KF.design_reference(mom, plans, return_p=True)
    assert des["status"].tolist() == [0, 0] and des["M"].dtype == F and des["K"].shape == (2, 2 * d, d)
    worst = 0.0
    for p, (Mw, Kw, c1, c2) in enumerate(design_linalg(mom, plans)):
        P = des["P"][p]
        assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P).min() > 0                  # symmetric in every bit, positive definite
        assert same_bits(des["M"][p], des["M64"][p].astype(F)) and same_bits(des["K"][p], des["K64"][p].astype(F))     # rounded once
        worst = max(worst, np.abs(des["M64"][p] - Mw).max(), np.abs(des["K64"][p] - Kw).max())
        print(f"D = {d} plan {p}: cond(G + lambda I) = {c1:.3e}, cond(H P- H^T + Q) = {c2:.3e}")
    print(f"D = {d}: max|M, K - linalg| before the rounding to f32 = {worst:.3e}")
    assert worst <= LINALG_BOUND[d]


def test_design_status_and_the_frozen_plans():
    a, y, groups, lo, span, rest = filter_case(60, 2, seed=9)
    c = KF.centre(lo, span, rest)
    mom = KF.moments_reference(a, y, groups, 3, c)
    few = KF.moments_reference(a[:6], y[:6], np.zeros(6, dtype=np.int64), 3, c)        # four samples < 2D + 1
    assert few["n"].tolist() == [4, 0, 0]
    des = KF.design_reference(few, [((0,), 1e-3, 1.0, 1.0, 4)])
    assert des["status"].tolist() == [1] and not des["M"].any() and not des["K"].any() and np.isinf(des["delta"][0])
    flat = KF.moments_reference(np.tile(a[:1], (40, 1)), np.tile(y[:1], (40, 1)), np.zeros(40, dtype=np.int64), 1, c)
    assert KF.design_reference(flat, [(1, 0.0, 1.0, 1.0, 4)])["status"].tolist() == [2]   # omega = 0: G is singular without a ridge
    # a plan's result does not depend on the plans beside it, nor on their T
    plans = [((0, 1, 2), 1e-3, 1.0, 1.0, 1), ((0, 1), 1e-3, 1.0, 0.25, 7), ((0, 1, 2), 1e-3, 1.0, 1.0, 3)]
    both = KF.design_reference(mom, plans)
    for i, p in enumerate(plans):
        one = KF.design_reference(mom, [p])
        assert all(same_bits(both[k][i:i + 1], one[k]) for k in ("M", "K", "delta", "status")), i
    assert KF.design_reference(mom, [])["M"].shape == (0, 4, 4)


def crafted_rows():
    """Two joints, lo 0, span 1, rest 1024 and 2048 (c = 0.25, 0.5) and a hand-made stable filter: rows that come before the
    start (a NaN, an infinity), the start, steps large enough to clamp both ways and to be rate-limited both ways, non-finite
    rows after the start (held), and rows with the class "none" """
    M = np.array([[0.5, 0.0, 0.4, 0.0], [0.0, 0.6, 0.0, 0.3], [-0.2, 0.0, 0.5, 0.0], [0.0, -0.1, 0.0, 0.6]], dtype=F)
    Kg = np.array([[0.5, 0.0], [0.1, 0.4], [0.2, 0.0], [0.0, 0.1]], dtype=F)
    lo, span, rest = np.zeros(2, dtype=F), np.ones(2, dtype=F), np.array([1024, 2048], dtype=np.int32)
    a = np.array([[np.nan, 0.3], [0.2, np.inf], [0.3, 0.6], [0.35, 0.62], [5.0, 4.0], [5.0, 4.0], [np.nan, 0.5], [0.4, -np.inf],
                  [-5.0, -4.0], [-5.0, -4.0], [0.5, 0.5], [0.5, 0.5], [0.52, 0.48], [0.9, 0.1], [0.9, 0.1], [0.2, 0.8]] * 2, dtype=F)
    a[16:] = a[16:] * F(0.9) + F(0.03)
    cls = np.where(np.arange(32) % 5 == 3, -1, 2).astype(np.int64)
    return M, Kg, lo, span, rest, a, cls


def test_filter_reference_gives_the_same_rows_for_any_cut():
    M, Kg, lo, span, rest, a, cls = crafted_rows()
    whole = KF.FilterReference(M, Kg, lo, span, rest, rate=600)
    filt, pose, angle = whole.push(a, cls)
    assert whole.events == EVENTS
    assert np.isnan(filt[:2]).all() and pose[:2].tolist() == [[600, 600], [1024, 1200]] and not np.isnan(filt[2:]).any()
    assert same_bits(filt[2], (a[2] - whole.c) + whole.c)                                 # the start: x = [o, 0]
    assert same_bits(filt[6], filt[5]) and same_bits(filt[7], filt[5])                    # held on non-finite rows
    assert np.abs(np.diff(pose.astype(np.int64), axis=0)).max() == 600 and pose.min() >= 0 and pose.max() <= 4096
    # one step by a scalar loop: row 3 from the state the start left
    x = np.concatenate([a[2] - whole.c, np.zeros(2, dtype=F)])
    o = a[3] - whole.c
    want = []
    for i in range(4):
        acc = F(0.0)
        for j in range(4):
            acc = F(acc + F(M[i, j] * x[j]))
        for j in range(2):
            acc = F(acc + F(Kg[i, j] * o[j]))
        want.append(acc)
    assert same_bits(filt[3], np.array(want[:2], dtype=F) + whole.c)
    for cut in (1, 3, 16, 17):
        ref = KF.FilterReference(M, Kg, lo, span, rest, rate=600)
        parts = [ref.push(a[s:s + cut], cls[s:s + cut]) for s in range(0, 32, cut)]
        got = [np.concatenate([p[i] for p in parts]) for i in range(3)]
        assert same_f32(got[0], filt) and same_bits(got[1], pose) and same_bits(got[2], angle), cut
        assert same_bits(ref.state()["x"], whole.state()["x"]) and same_bits(ref.state()["out"], whole.state()["out"])
    nocls = KF.FilterReference(M, Kg, lo, span, rest, rate=600)
    f2, p2, _ = nocls.push(a)
    assert "none" not in nocls.events and same_f32(f2, filt) and not same_bits(p2, pose)  # the class moves the pose, not the filter
    free = KF.FilterReference(M, Kg, lo, span, rest)                                      # no rate limit: pose = q
    f3, p3, _ = free.push(a)
    t = (f3 - lo) / span
    assert np.array_equal(p3[2:], np.rint(np.clip(t[2:], 0, 1) * F(4096)).astype(np.int32))


def test_sweep_reference_is_filter_reference_restarted_at_every_run():
    a, y, groups, lo, span, rest = filter_case(60, 3, seed=4)
    c = KF.centre(lo, span, rest)
    a[25] = np.nan                                             # a hold inside a run
    a[40] = np.nan                                             # the first row of a run: it starts one row later
    assert groups[39] == 1 and groups[40] == 2
    des = KF.design_reference(KF.moments_reference(np.nan_to_num(a), y, groups, 3, c), [((0, 1, 2), 1e-3, 1.0, 1.0, 16)] * 2)
    masks = [0b101, 0b010]
    sums, filt = KF.sweep_reference(a, y, groups, masks, des["M"], des["K"], c, return_filtered=True)
    for p, mask in enumerate(masks):
        want = np.full((60, 3), np.nan, dtype=F)
        runs, k = [], 0
        while k < 60:
            e = k
            while e < 60 and groups[e] == groups[k]:
                e += 1
            if groups[k] >= 0 and (mask >> groups[k]) & 1:
                runs.append((k, e))
            k = e
        jit = np.zeros(3)
        for s, e in runs:
            ref = KF.FilterReference(des["M"][p], des["K"][p], lo, span, rest)
            want[s:e] = ref.push(a[s:e])[0]
            d = np.diff(want[s:e].astype(np.float64), axis=0)
            jit += np.nansum(d * d, axis=0)
        assert same_f32(filt[p], want), p
        has = ~np.isnan(want[:, 0])
        assert np.array_equal(sums[p, :, 0], np.full(3, has.sum())) and has.sum() == sum(e - s for s, e in runs) - (1 if p == 0 else 0)
        score = K.score_reference(want[None][:, has], y[has], groups[has], [mask])[0]
        assert same_bits(sums[p, :, :7], score)
        assert np.allclose(sums[p, :, 7], jit, rtol=1e-12)
    assert len(runs) == 2                                      # group 1: two runs around the unused window
    bare = KF.unfiltered_sums(a, y, groups, [0b010])
    assert same_bits(bare[0, :, :7], K.score_reference(a[None], y, groups, [0b010])[0])


@pytest.fixture(scope="module")
def person():
    rec = K.kinematics_recording(4, 3, 12, 3)
    out = {}
    for lag in (0, 2):
        y = K.window_targets(rec["glove"], 0, lag)
        n = int(y.shape[0])
        rep = (rec["rep"][:n], rec["n_rep"])
        a = KF.crossfit_reference(rec["u"][:n], y, rep, 0.01)
        lo, span, rest = K.limits(y, rec["cls"][:n], 0)
        fit = K.PoseFit(np.zeros((1, 3, 512), dtype=F), np.zeros((1, 3), dtype=F), [0], [((0, 1, 2), 0.01)], {}, lo, span, rest, lag)
        out[lag] = (a, y, rep, fit)
    return out


def test_on_the_synthetic_person_the_recursion_converges_and_the_filter_helps(person):
    a, y, rep, fit = person[0]
    out = KF.pick_filter_reference(a, y, rep, fit, kappas=(0.25, 1.0, 4.0), iters=128)
    print("lag 0: rho, kappa, RMSE, jitter\n", out["table"], "\ndelta", out["delta"].max())
    assert out["ok"].all() and out["delta"].shape == (3, 3) and out["delta"].max() < 1e-10
    assert out["table"].shape == (4, 4) and np.isnan(out["table"][0, :2]).all()
    assert out["table"][1:, 2].min() < out["table"][0, 2]       # the best kappa is below the unfiltered readout
    assert out["pick"] == out["best_filter"] and out["kappa"] == out["table"][out["pick"], 1]
    # the unfiltered row is the score of a itself
    groups = rep[0]
    bare = K.metrics(K.score_reference(a[None], y, groups, [0b111]))["rmse_mean"][0]
    assert np.isclose(out["table"][0, 2], bare, rtol=1e-12)
    a2, y2, rep2, fit2 = person[2]
    out2 = KF.pick_filter_reference(a2, y2, rep2, fit2, kappas=(0.25, 1.0, 4.0), iters=128)
    print("lag 2: rho, kappa, RMSE, jitter\n", out2["table"])
    assert out2["delta"].max() < 1e-10 and out2["table"][out2["pick"], 2] <= out2["table"][0, 2]


def test_the_tie_rule_of_the_pick():
    rows = [(1.0, 0.25), (1.0, 1.0), (1.0, 4.0)]
    fold = np.zeros((2, 3, 2, 8))
    fold[..., 0] = 10.0
    fold[..., 6] = 40.0                                        # every filtered row: RMSE 2
    bare = np.zeros((2, 2, 8))
    bare[..., 0], bare[..., 6] = 10.0, 40.0
    ok, delta = np.zeros((2, 3), dtype=np.int32), np.zeros((2, 3))
    assert KF._pick_tables(fold, ok, delta, bare, rows, 2)["pick"] == 0                   # equal: the unfiltered row first
    bare[..., 6] = 41.0
    out = KF._pick_tables(fold, ok, delta, bare, rows, 2)
    assert out["pick"] == 3 and out["kappa"] == 4.0 and out["rho"] == 1.0                 # then the larger kappa
    ok[1, 2] = 3
    assert KF._pick_tables(fold, ok, delta, bare, rows, 2)["pick"] == 2                   # a row with a failed fold is never picked
    fold[:, 0, :, 6] = 30.0
    assert KF._pick_tables(fold, ok, delta, bare, rows, 2)["pick"] == 1


def test_the_python_layer_refuses_bad_arguments():
    a, y, groups, lo, span, rest = filter_case(30, 2, seed=6)
    c = KF.centre(lo, span, rest)
    with pytest.raises(ValueError, match="D in 1..32"):
        KF.moments_reference(np.zeros((5, 33), dtype=F), np.zeros((5, 33), dtype=F), None, 1, np.zeros(33))
    with pytest.raises(ValueError, match="targets"):
        KF.moments_reference(a, y[:-1], groups, 3, c)
    with pytest.raises(ValueError, match="one entry per window"):
        KF.moments_reference(a, y, groups[:-1], 3, c)
    with pytest.raises(ValueError, match="centre"):
        KF.moments_reference(a, y, groups, 3, c[:1])
    with pytest.raises(ValueError, match="centre"):
        KF.moments_reference(a, y, groups, 3, np.array([0.0, np.nan]))
    mom = KF.moments_reference(a, y, groups, 3, c)
    good = ((0, 1), 1e-3, 1.0, 1.0, 8)
    for bad, what in (((0, 1), "a plan is"), (((0, 3),) + good[1:], "groups"), ((8,) + good[1:], "mask"), (good[:1] + (-1.0,) + good[2:], "lam"),
                      (good[:2] + (0.0,) + good[3:], "rho"), (good[:3] + (float("nan"),) + good[4:], "kappa"), (good[:4] + (0,), "T"),
                      (good[:4] + (1025,), "T"), (good[:4] + (2.0,), "T")):
        with pytest.raises(ValueError, match=what):
            KF.design_reference(mom, [bad])
    with pytest.raises(ValueError, match="256"):
        KF.design_reference(mom, [good] * 257)
    with pytest.raises(ValueError, match="mom"):
        KF.design_reference(dict(mom, E=np.zeros((3, 3, 3))), [good])
    des = KF.design_reference(mom, [good])
    with pytest.raises(ValueError, match="M \\(2D, 2D\\)"):
        KF.FilterReference(des["M"], des["K"], lo, span, rest)
    with pytest.raises(ValueError, match="2D"):
        KF.FilterReference(des["M"][0][:3], des["K"][0], lo, span, rest)
    with pytest.raises(ValueError, match="rate"):
        KF.FilterReference(des["M"][0], des["K"][0], lo, span, rest, rate=0)
    with pytest.raises(ValueError, match="span"):
        KF.FilterReference(des["M"][0], des["K"][0], lo, -span, rest)
    ref = KF.FilterReference(des["M"][0], des["K"][0], lo, span, rest)
    with pytest.raises(ValueError, match="a must be"):
        ref.push(a[:, :1])
    with pytest.raises(ValueError, match="cls"):
        ref.push(a, np.zeros(3))
    with pytest.raises(ValueError, match="one test mask per plan"):
        KF.sweep_reference(a, y, groups, [1, 2], des["M"], des["K"], c)
    with pytest.raises(ValueError, match="two repetitions"):
        KF.crossfit_reference(np.zeros((30, 512), dtype=F), y, (np.zeros(30, dtype=np.int64), 1))
    with pytest.raises(ValueError, match="repetition of every window"):
        KF.crossfit_reference(np.zeros((30, 512), dtype=F), y, None)
    fit = K.PoseFit(np.zeros((1, 2, 512), dtype=F), np.zeros((1, 2), dtype=F), [0], [((0,), 0.1)], {}, lo, span, rest)
    with pytest.raises(ValueError, match="two repetitions"):
        KF.pick_filter_reference(a, y, (np.zeros(30, dtype=np.int64), 1), fit)
    with pytest.raises(ValueError, match="at least one value"):
        KF.pick_filter_reference(a, y, (groups, 3), fit, kappas=())
    with pytest.raises(ValueError, match="256 plans"):
        KF.pick_filter_reference(a, y, (groups, 3), fit, kappas=np.linspace(0.1, 1, 43), rhos=(1.0, 2.0))
    ff = KF.FilterFit(des["M"], des["K"], des["delta"], [2], [good], {}, c, fit)
    with pytest.raises(ValueError, match="no filter"):
        ff.install(None, 0)
    with pytest.raises(IndexError):
        ff.install(None, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries: every refusal returns before any device call
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
    for n in ("cp_online_kf_design_bytes", "cp_online_kf_workspace_bytes"):
        assert hasattr(raw, n) and n in _lib.SYMBOLS and re.search(r"\bsize_t\s+%s\s*\(" % n, hdr), n
    for name in ("CP_ONLINE_KF_MAX_ITERS", "CP_ONLINE_KF_PLANS_PER_LAUNCH", "CP_ONLINE_KF_SUMS"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(_lib, name), name
    assert int(re.search(r"#define CP_VERSION (\d+)", text).group(1)) == 112
    for struct in (_lib.cp_online_kf_plan, _lib.cp_online_kf_config):
        body = hdr[hdr.index("typedef struct %s {" % struct.__name__):hdr.index("} %s;" % struct.__name__)]
        assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in struct._fields_]
    assert ctypes.sizeof(_lib.cp_online_kf_plan) == 32
    a256 = lambda n: (n + 255) // 256 * 256
    assert lib.cp_online_kf_workspace_bytes(0) == lib.cp_online_kf_workspace_bytes(1) == a256(4 * KF._STATE_WORDS)
    assert lib.cp_online_kf_workspace_bytes(256) == a256(256 * 4 * KF._STATE_WORDS) and KF._STATE_WORDS == 22792
    assert lib.cp_online_kf_design_bytes(1) == 8 * (64 * 64 + 32 * 32) and lib.cp_online_kf_design_bytes(256) == 128 * lib.cp_online_kf_design_bytes(1)


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory for every pointer: each refusal returns before a launch, which on a machine without a GPU would fail otherwise"""
    from contrastiveprosthetics_amd import _lib
    buf = ctypes.create_string_buffer(1 << 20)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 40
    f20 = lambda *v: (ctypes.c_float * 20)(*(list(v) + [1.0] * (20 - len(v))))

    def err(rc, entry, what, code=ERR_ARG):
        assert rc == code, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    name = "cp_online_kf_moments"
    mo = lambda a=p, y=p, group=p, n=8, d=20, r=2, c=f20(), G=p, Cm=p, S=p, E=p, count=p: \
        lib.cp_online_kf_moments(a, y, group, n, d, r, c, G, Cm, S, E, count, None)
    for n in (-1, (1 << 24) + 1):
        err(mo(n=n), name, "n_rows")
    for d in (0, 33):
        err(mo(d=d), name, "n_joints")
    for r in (0, 17):
        err(mo(r=r), name, "n_groups")
    for arg in ("a", "y", "group", "G", "Cm", "S", "E", "count", "c"):
        err(mo(**{arg: None}), name, "required")
    for arg in ("a", "y", "group", "G", "Cm", "S", "E", "count"):
        err(mo(**{arg: p + 2}), name, "misaligned")
    err(mo(G=p + 4), name, "misaligned")
    for bad in (float("nan"), float("inf")):
        err(mo(c=f20(0.0, bad)), name, "centre must be finite")

    name = "cp_online_kf_design"

    def table(**kw):
        t = (_lib.cp_online_kf_plan * 2)()
        for i in range(2):
            t[i].groups, t[i].iters, t[i].lam, t[i].rho, t[i].kappa = 3, 8, 1e-3, 1.0, 1.0
        for k, v in kw.items():
            setattr(t[1], k, v)
        return t

    de = lambda G=p, Cm=p, S=p, E=p, count=p, d=20, r=2, plans=table(), P=2, M=p, Kg=p, delta=p, status=p, sc=p, nb=big: \
        lib.cp_online_kf_design(G, Cm, S, E, count, d, r, plans, P, M, Kg, delta, status, sc, nb, None)
    for d in (0, 33):
        err(de(d=d), name, "n_joints")
    for r in (0, 17):
        err(de(r=r), name, "n_groups")
    for P in (-1, 257):
        err(de(P=P), name, "n_plans")
    assert de(P=0) == 0
    for arg in ("G", "Cm", "S", "E", "count", "plans", "M", "Kg", "delta", "status", "sc"):
        err(de(**{arg: None}), name, "required")
    for arg in ("G", "Cm", "S", "E", "count", "M", "Kg", "delta", "status", "sc"):
        err(de(**{arg: p + 2}), name, "misaligned")
    err(de(delta=p + 4), name, "misaligned")
    err(de(sc=p + 64), name, "misaligned")
    err(de(plans=table(groups=4)), name, "mask")
    for iters in (0, 1025):
        err(de(plans=table(iters=iters)), name, "iters outside 1..1024")
    for lam in (-1.0, float("nan"), float("inf")):
        err(de(plans=table(lam=lam)), name, "lam")
    for v in (0.0, -1.0, float("nan"), float("inf")):
        err(de(plans=table(rho=v)), name, "rho")
        err(de(plans=table(kappa=v)), name, "kappa")
    err(de(nb=lib.cp_online_kf_design_bytes(2) - 256), name, "scratch too small", ERR_WORKSPACE)

    name = "cp_online_kf_sweep"
    masks = (ctypes.c_uint32 * 4)(1, 2, 4, 3)
    sw = lambda a=p, y=p, group=p, n=8, d=20, masks=masks, P=4, M=p, Kg=p, c=f20(), sums=p, filt=None: \
        lib.cp_online_kf_sweep(a, y, group, n, d, masks, P, M, Kg, c, sums, filt, None)
    for n in (-1, (1 << 24) + 1):
        err(sw(n=n), name, "n_rows")
    for d in (0, 33):
        err(sw(d=d), name, "n_joints")
    for P in (-1, 257):
        err(sw(P=P), name, "n_plans")
    assert sw(P=0) == 0
    for arg in ("a", "y", "group", "masks", "M", "Kg", "sums", "c"):
        err(sw(**{arg: None}), name, "required")
    for arg in ("a", "y", "group", "M", "Kg", "sums", "filt"):
        err(sw(**{arg: p + 2}), name, "misaligned")
    err(sw(sums=p + 4), name, "misaligned")
    err(sw(masks=(ctypes.c_uint32 * 4)(1, 2, 1 << 16, 3)), name, "mask")
    err(sw(c=f20(float("nan"))), name, "centre must be finite")

    cfg = _lib.cp_online_kf_config()
    cfg.rate = 4096
    ws_bytes = lib.cp_online_kf_workspace_bytes(3)
    assert ws_bytes <= 1 << 19
    lo, span, rest = f20(0.0), f20(1.0), (ctypes.c_int32 * 20)(*([0] * 20))

    def entries(c=cfg, s=3, ws=p, nb=ws_bytes):
        """every stage entry with the same config, stream count and workspace"""
        cp = ctypes.byref(c) if c is not None else None
        return [("cp_online_kf_set_model", lib.cp_online_kf_set_model(cp, s, ws, nb, 0, p, p, 20, lo, span, rest, p, p, None)),
                ("cp_online_kf_reset", lib.cp_online_kf_reset(cp, s, ws, nb, -1, None)),
                ("cp_online_kf_push", lib.cp_online_kf_push(cp, s, ws, nb, p, 0, 512, None, p, p, 8, p, p, p, p, None))]

    def every(what, code=ERR_ARG, **kw):
        for name, rc in entries(**kw):
            assert rc == code, (name, what, rc)

    every("config", c=None)
    every("workspace", ws=None)
    for s in (0, 257):
        every("n_streams", s=s)
    for rate in (0, 4097):
        c2 = _lib.cp_online_kf_config()
        c2.rate = rate
        every("rate", c=c2)
        assert b"cp_online_kf_push" in lib.cp_last_error() and b"rate outside 1..4096" in lib.cp_last_error()
    every("aligned", ws=p + 64)
    assert b"not 256-byte aligned" in lib.cp_last_error()
    every("too small", code=ERR_WORKSPACE, nb=ws_bytes - 256)
    assert b"workspace too small" in lib.cp_last_error()

    name = "cp_online_kf_set_model"
    sm = lambda index=0, W=p, b=p, d=20, lo=lo, span=span, rest=rest, M=p, Kg=p: \
        lib.cp_online_kf_set_model(ctypes.byref(cfg), 3, p, ws_bytes, index, W, b, d, lo, span, rest, M, Kg, None)
    for index in (-1, 3):
        err(sm(index=index), name, "stream index")
    for d in (0, 33):
        err(sm(d=d), name, "n_joints outside 1..32")
    for arg in ("W", "b", "lo", "span", "rest", "M", "Kg"):
        err(sm(**{arg: None}), name, "required")
    err(sm(W=p + 4), name, "misaligned")
    for arg in ("b", "M", "Kg"):
        err(sm(**{arg: p + 2}), name, "misaligned")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        err(sm(span=f20(1.0, bad)), name, "span")
    err(sm(lo=f20(0.0, float("inf"))), name, "lo")
    for bad in (-1, 4097):
        err(sm(rest=(ctypes.c_int32 * 20)(0, bad)), name, "rest")

    name = "cp_online_kf_reset"
    for index in (-2, 3):
        err(lib.cp_online_kf_reset(ctypes.byref(cfg), 3, p, ws_bytes, index, None), name, "stream index")

    name = "cp_online_kf_push"
    pu = lambda tail=p, dtype=0, ldt=512, cls=None, row0=p, m=p, rows=8, raw=p, filt=p, pose=p, angle=p: \
        lib.cp_online_kf_push(ctypes.byref(cfg), 3, p, ws_bytes, tail, dtype, ldt, cls, row0, m, rows, raw, filt, pose, angle, None)
    err(pu(dtype=2), name, "dtype")
    for rows in (-1, 65537):
        err(pu(rows=rows), name, "total_rows")
    assert pu(rows=0) == 0 and pu(rows=0, tail=None) == 0      # an empty call
    err(pu(ldt=511), name, "ldt")
    for arg in ("tail", "row0", "m", "raw", "filt", "pose", "angle"):
        err(pu(**{arg: None}), name, "required")
    for arg in ("tail", "cls", "row0", "m", "raw", "filt", "pose", "angle"):
        err(pu(**{arg: p + 2}), name, "misaligned")
    err(pu(tail=p + 8), name, "misaligned")
