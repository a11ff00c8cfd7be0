"""The closed-form head fit without a GPU (contrastiveprosthetics_amd/readout.py, include/cpnative.h cp_online_readout_*): the
numpy definitions `fit_reference` and `apply_reference` against numpy.linalg.solve, the properties the definition promises, the
point of the synthetic person, argument validation of the Python layer, and the binding and host checks of the C entries."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import readout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG, ERR_WORKSPACE = 10001, 10002
F = np.float32
ENTRIES = ["cp_online_readout_moments", "cp_online_readout_solve", "cp_online_readout_apply"]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def small_case(n, k=3, seed=0, n_groups=3, bf16=False):
    """n windows of rectified tail inputs over k slots and n_groups groups, with unused windows (slot -1) among them"""
    rng = np.random.default_rng(seed)
    u = np.maximum(rng.standard_normal((n, 512)) + 0.2, 0.0).astype(F)
    if bf16:
        u = R.round_bf16(u).astype(F)
    slots = rng.integers(0, k, size=n)
    slots[rng.random(n) < 0.15] = -1
    groups = rng.integers(0, n_groups, size=n)
    targets = R.unit_targets(rng.standard_normal((k, 16)).astype(F))
    return u, slots.astype(np.int64), groups.astype(np.int64), targets


@pytest.fixture(scope="module")
def case100():
    u, slots, groups, targets = small_case(100, seed=1)
    fit = R.fit_reference(u, slots, targets, plans=[((0, 1, 2), 1e-2), ((0, 2), 1.0)], groups=groups, n_groups=3)
    for v in (u, slots, groups, targets, *[fit[key] for key in ("W", "b", "X", "G", "C", "weights")]):
        v.setflags(write=False)
    return u, slots, groups, targets, fit


# ---------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------
def test_fit_reference_solves_the_system_numpy_builds(case100):
    """The same system built by X.T @ diag(w) @ X and solved by numpy.linalg.solve.  Compared by the normal-equation residual
    |A X - B|_inf of the float64 solution.  The bound: a Cholesky solve is backward stable with |dA| <= g(3n+1) |L||L^T|
    (Higham, Accuracy and Stability, th. 10.4), and | |L||L^T| |_inf <= n |A|_inf, so the residual stays within
    (3n+1) n u |A|_inf |X|_inf; the sequential moments differ from the BLAS ones by at most (N + 2) u per element relative to
    sums of absolute values (all terms of G are >= 0: u is rectified), which adds (N + 2) u (|A|_inf |X|_inf + |B|_inf);
    n = 513, u = 2^-53."""
    u, slots, groups, targets, fit = case100
    n_w, n, eps = u.shape[0], 513, 2.0 ** -53
    xm = np.concatenate([u.astype(np.float64), np.ones((n_w, 1))], axis=1)
    w = fit["weights"]
    assert same_bits(w, R.window_weights(slots, 3, True, groups))
    for t, (grp, lam) in enumerate([((0, 1, 2), 1e-2), ((0, 2), 1.0)]):
        wt = np.where(np.isin(groups, grp) & (slots >= 0), w, 0.0)
        a = xm.T @ (wt[:, None] * xm) + lam * np.diag(np.r_[np.ones(512), 0.0])
        b = xm.T @ (wt[:, None] * targets.astype(np.float64)[np.maximum(slots, 0)])
        assert fit["status"][t] == 0
        x = fit["X"][t]
        a_inf, x_inf, b_inf = np.abs(a).sum(axis=1).max(), np.abs(x).sum(axis=1).max(), np.abs(b).sum(axis=1).max()
        bound = ((3 * n + 1) * n * a_inf * x_inf + (n_w + 2) * (a_inf * x_inf + b_inf)) * eps
        res = np.abs(a @ x - b).sum(axis=1).max()
        lib_res = np.abs(a @ np.linalg.solve(a, b) - b).sum(axis=1).max()
        print(f"plan {t}: residual {res:.3e}, numpy.linalg.solve {lib_res:.3e}, bound {bound:.3e}")
        assert res <= bound, (t, res, bound)
        assert same_bits(fit["W"][t], x[:512].T.astype(F)) and same_bits(fit["b"][t], x[512].astype(F))
        wrong = x.copy()
        wrong[7] *= 1.0 + 1e-4                                 # (an a-priori bound: it tells a row that is off in the fourth digit)
        assert np.abs(a @ wrong - b).sum(axis=1).max() > bound


def test_moments_do_not_depend_on_how_the_recording_is_cut(case100):
    """there is no cut in the definition: a group's windows in order reproduce it, whatever else lies between them"""
    u, slots, groups, targets, fit = case100
    w = fit["weights"]
    for r in range(3):
        sel = np.nonzero(groups == r)[0]
        g1, c1 = R.moments_reference(u[sel], slots[sel], w[sel], targets)
        assert same_bits(g1[0], fit["G"][r]) and same_bits(c1[0], fit["C"][r])
    assert same_bits(fit["G"], np.transpose(fit["G"], (0, 2, 1)))
    # element by element: a scalar loop in window order
    r, a, b, d = 1, 37, 512, 5
    g = c = np.float64(0.0)
    for i in np.nonzero((groups == r) & (slots >= 0))[0]:
        xa = np.float64(u[i, a])
        g = g + w[i] * (xa * np.float64(1.0))
        c = c + w[i] * (xa * np.float64(targets[slots[i], d]))
    assert g == fit["G"][r, a, b] == fit["G"][r, b, a] and c == fit["C"][r, a, d]


def test_the_order_of_a_plans_groups_does_not_matter(case100):
    u, slots, groups, targets, fit = case100
    one = R.solve_reference(fit["G"], fit["C"], [((2, 0), 1.0), (0b101, 1.0)])
    assert same_bits(one[0][0], fit["W"][1]) and same_bits(one[0][1], fit["W"][1])
    assert same_bits(one[1][0], fit["b"][1]) and same_bits(one[1][1], fit["b"][1])


def test_cholesky_is_the_scalar_loop_of_the_docstring():
    rng = np.random.default_rng(3)
    m = rng.standard_normal((40, 12))
    a = m.T @ m + 0.1 * np.eye(12)
    low, status = R.cholesky_reference(a)
    assert status == 0
    for i in range(12):
        for j in range(i + 1):
            r = a[i, j]
            for k in range(j):
                r = r - low[i, k] * low[j, k]
            assert low[i, j] == (np.sqrt(r) if i == j else r / low[j, j]), (i, j)
    a[5, 5] = -1.0
    assert R.cholesky_reference(a)[1] == 6


def test_nothing_to_fit_fails_at_the_first_pivot():
    u = np.zeros((20, 512), dtype=F)
    slots = np.arange(20) % 2
    fit = R.fit_reference(u, slots, R.unit_targets(np.eye(2, 16, dtype=F)), ridge=[0.0, 0.5])
    assert fit["status"].tolist() == [1, 0]
    assert not fit["W"][0].any() and not fit["b"][0].any()
    assert not fit["W"][1].any()                               # u = 0: the ridge leaves the bias alone to fit the mean target
    assert np.allclose(fit["b"][1], R.unit_targets(np.eye(2, 16, dtype=F)).mean(axis=0), atol=1e-6)


def test_weights_sum_to_one():
    rng = np.random.default_rng(4)
    slots = rng.integers(-1, 5, size=333)
    slots[slots == 3] = 0                                      # a slot without windows
    for balanced in (True, False):
        w = R.window_weights(slots, 5, balanced)
        assert abs(w.sum() - 1.0) < 333 * 2.0 ** -52 and (w[slots < 0] == 0).all() and (w[slots >= 0] > 0).all()
    w = R.window_weights(slots, 5, True)
    assert w[slots == 1][0] == 1.0 / (4.0 * (slots == 1).sum())


def test_apply_reference_is_the_projection_normalised():
    rng = np.random.default_rng(5)
    u = np.maximum(rng.standard_normal((33, 512)), 0).astype(F)
    W, b = (0.05 * rng.standard_normal((2, 16, 512))).astype(F), rng.standard_normal((2, 16)).astype(F)
    for dtype, tol in (("f32", 2e-6), ("bf16", 2e-6)):
        uu = u if dtype == "f32" else R.round_bf16(u).astype(F)
        z = R.apply_reference(uu, W, b, dtype)
        assert z.shape == (2, 33, 16) and z.dtype == F
        wt = W.astype(np.float64) if dtype == "f32" else R.round_bf16(W)
        want = np.einsum("nk,pdk->pnd", uu.astype(np.float64), wt) + b[:, None, :]
        want /= np.linalg.norm(want, axis=2, keepdims=True)
        assert np.abs(z - want).max() < tol
        assert same_bits(R.apply_reference(uu, W[1], b[1], dtype), z[1])


# ---------------------------------------------------------------------------------------------------------------------------
# the synthetic person
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_fit_gains_a_tenth_of_the_held_out_windows_on_the_synthetic_person():
    """8 classes (two pairs of near-twins), 4 repetitions, 40 windows per segment, noise 0.9, wander 0.3, seed 0.  Leave one
    repetition out through the definitions at ridge 0.1: the raw hits of rows enrolled in the fitted space against rows
    enrolled under the unfitted projection."""
    p = R.readout_recording(8, 4, 40, seed=0, noise=0.9, wander=0.3)
    u, slots = p["u"], p["slots"]
    assert u.shape == (1280, 512) and (u >= 0).all() and same_bits(p["rep"], H.repetitions(slots, None)[0].astype(np.int64))
    emb0 = R.apply_reference(u, p["W0"], p["b0"], "f32")
    table = R.enrolled_rows_reference(emb0, slots, 8, np.ones(1280, dtype=bool))
    out = R.pick_ridge_reference(u, slots, np.arange(8), table, emb0, ridges=[0.1])
    base, n_cue = out["baseline"], int(out["n_cue"][0])
    print(f"held-out raw hits {base['raw_hit']} -> {int(out['raw_hit'][0])} of {n_cue}; voted {base['voted_hit']} -> {int(out['voted_hit'][0])}")
    assert n_cue == base["n_cue"] == 1280 and out["best"] == 0 and out["ridge"] == 0.1
    assert 10 * (int(out["raw_hit"][0]) - base["raw_hit"]) >= n_cue


# ---------------------------------------------------------------------------------------------------------------------------
# argument validation of the Python layer
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_python_layer_refuses_bad_arguments():
    u, slots, groups, targets = small_case(20, seed=6)
    w = R.window_weights(slots, 3)
    with pytest.raises(ValueError, match="512"):
        R.moments_reference(u[:, :100], slots, w, targets)
    with pytest.raises(ValueError, match="one integer entry per window"):
        R.moments_reference(u, slots[:5], w, targets)
    with pytest.raises(ValueError, match="number of groups"):
        R.moments_reference(u, slots, w, targets, groups, n_groups=17)
    with pytest.raises(ValueError, match="below the number of groups"):
        R.moments_reference(u, slots, w, targets, groups, n_groups=2)
    with pytest.raises(ValueError, match="float32"):
        R.moments_reference(u.astype(np.float64) + 1e-12, slots, w, targets)
    G, Cm = np.zeros((2, 513, 513)), np.zeros((2, 513, 16))
    for plans, what in (([((0,), -1.0)], "ridge"), ([((0,), float("nan"))], "ridge"), ([((2,), 1.0)], "training group"),
                        ([(4, 1.0)], "mask"), ([(0, 1.0, 2)], "pair"), ([((0,), 1.0)] * 257, "at most 256")):
        with pytest.raises(ValueError, match=what):
            R.solve_reference(G, Cm, plans)
    with pytest.raises(ValueError, match="dtype"):
        R.apply_reference(u, np.zeros((16, 512), F), np.zeros(16, F), "fp8")
    with pytest.raises(ValueError, match="W"):
        R.apply_reference(u, np.zeros((16, 100), F), np.zeros(16, F))
    with pytest.raises(ValueError, match="ridges"):
        R._check_ridges([])
    fit = R.Readout(np.zeros((2, 16, 512), F), np.zeros((2, 16), F), [0, 7], [((0,), 0.1), ((0,), 0.0)], {2: 30}, [2], "f32")

    class Multi:
        class_ids = [None, None]

        def set_projection(self, W, b):
            raise AssertionError("never installed")

    with pytest.raises(Exception, match="share one projection"):
        fit.install(Multi(), 0)

    class Single:
        class_ids, got = None, None

        def set_projection(self, W, b):
            self.got = (W, b)

    dec = Single()
    with pytest.raises(ValueError, match="positive definite"):
        fit.install(dec, 1)
    with pytest.raises(IndexError):
        fit.install(dec, 2)
    assert dec.got is None
    fit.install(dec, 0)
    assert dec.got[0].shape == (16, 512) and dec.got[1].shape == (16,)


def test_the_tie_rule_of_the_pick():
    lam = np.array([0.01, 0.1, 1.0])
    out = R._pick(2, lam, [5, 6, 6, 5, 6, 6], [4, 7, 7, 4, 7, 7], [10] * 6, [0] * 6, [(3, 3, 10), (2, 2, 10)])
    assert out["best"] == 2 and out["ridge"] == 1.0 and out["voted_hit"].tolist() == [8, 14, 14] and out["n_cue"].tolist() == [20] * 3
    assert out["baseline"] == dict(raw_hit=5, voted_hit=5, n_cue=20)
    out = R._pick(2, lam, [5, 6, 6, 5, 6, 6], [4, 7, 7, 4, 7, 7], [10] * 6, [0, 0, 0, 0, 0, 3], [(3, 3, 10), (2, 2, 10)])
    assert out["best"] == 1 and out["voted_hit"].tolist() == [8, 14, -1] and out["raw_hit"].tolist() == [10, 12, -1]


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
    names = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", hdr))
    assert set(_lib.SYMBOLS) == names
    raw = ctypes.CDLL(LIB)
    for n in ENTRIES:
        assert hasattr(raw, n) and n in _lib.SYMBOLS, n
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert m and len(m.group(1).split(",")) == len(_lib.SYMBOLS[n][1]), n
    assert hasattr(raw, "cp_online_readout_scratch_bytes") and "cp_online_readout_scratch_bytes" in _lib.SYMBOLS
    for name in ("CP_ONLINE_READOUT_MAX_GROUPS", "CP_ONLINE_READOUT_MAX_PLANS", "CP_ONLINE_READOUT_STAGE", "CP_ONLINE_READOUT_X"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(_lib, name), name
    assert (R.MAX_GROUPS, R.MAX_PLANS, R.X) == (16, 256, 513)
    a256 = lambda n: (n + 255) // 256 * 256
    sb = lib.cp_online_readout_scratch_bytes
    assert sb(0, 0, 0) == sb(1, 1, 1) == a256(513 * 520 * 8)
    assert sb(100000, 16, 1) == a256(100000 * 16 * 4) + 256                 # the index lists and their lengths
    assert sb(100, 3, 7) == a256(7 * 513 * 520 * 8)                         # a matrix per plan


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory for every pointer: each refusal returns before a launch, which on a machine without a GPU would fail otherwise"""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 40

    def err(rc, entry, what, code=ERR_ARG):
        assert rc == code, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    name = "cp_online_readout_moments"
    mo = lambda u=p, dtype=0, n=8, slot=p, group=p, w=p, t=p, k=3, r=2, G=p, Cm=p, sc=p, nb=big: \
        lib.cp_online_readout_moments(u, dtype, n, slot, group, w, t, k, r, G, Cm, sc, nb, None)
    err(mo(dtype=2), name, "dtype")
    for n in (-1, (1 << 24) + 1):
        err(mo(n=n), name, "n_rows")
    for k in (0, 65):
        err(mo(k=k), name, "n_classes")
    for r in (0, 17):
        err(mo(r=r), name, "n_groups")
    for arg in ("u", "slot", "group", "w", "t", "G", "Cm", "sc"):
        err(mo(**{arg: None}), name, "required")
    for arg in ("u", "slot", "group", "w", "t", "G", "Cm", "sc"):
        err(mo(**{arg: p + 2}), name, "misaligned")
    err(mo(w=p + 4), name, "misaligned")
    err(mo(nb=256), name, "scratch too small", ERR_WORKSPACE)

    name = "cp_online_readout_solve"
    masks, lam = (ctypes.c_uint32 * 4)(1, 2, 3, 3), (ctypes.c_double * 4)(0.0, 0.1, 1.0, 10.0)
    so = lambda G=p, Cm=p, r=2, masks=masks, lam=lam, n=4, W=p, b=p, st=p, sc=p, nb=big: \
        lib.cp_online_readout_solve(G, Cm, r, masks, lam, n, W, b, st, sc, nb, None)
    for r in (0, 17):
        err(so(r=r), name, "n_groups")
    for n in (-1, 257):
        err(so(n=n), name, "n_plans")
    assert so(n=0) == 0 and so(n=0, G=None, sc=None) == 0      # an empty call
    for arg in ("G", "Cm", "masks", "lam", "W", "b", "st", "sc"):
        err(so(**{arg: None}), name, "required")
    for arg in ("G", "Cm", "W", "b", "st", "sc"):
        err(so(**{arg: p + 2}), name, "misaligned")
    err(so(masks=(ctypes.c_uint32 * 4)(1, 2, 4, 3)), name, "mask")
    for bad in (-0.5, float("nan"), float("inf")):
        err(so(lam=(ctypes.c_double * 4)(0.0, bad, 1.0, 1.0)), name, "ridge")
    err(so(nb=4 * 513 * 520 * 8 - 1), name, "scratch too small", ERR_WORKSPACE)

    name = "cp_online_readout_apply"
    ap = lambda u=p, dtype=1, n=8, W=p, b=p, P=2, out=p, sc=p, nb=big: lib.cp_online_readout_apply(u, dtype, n, W, b, P, out, sc, nb, None)
    err(ap(dtype=-1), name, "dtype")
    for n in (-1, (1 << 24) + 1):
        err(ap(n=n), name, "n_rows")
    for P in (-1, 257):
        err(ap(P=P), name, "n_plans")
    assert ap(n=0) == 0 and ap(P=0) == 0 and ap(n=0, u=None) == 0
    for arg in ("u", "W", "b", "out", "sc"):
        err(ap(**{arg: None}), name, "required")
    for arg in ("u", "W", "b", "out", "sc"):
        err(ap(**{arg: p + 2}), name, "misaligned")
    err(ap(nb=2 * 8192 * 4 - 1), name, "scratch too small", ERR_WORKSPACE)
