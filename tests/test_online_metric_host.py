"""The user metric without a GPU (contrastiveprosthetics_amd/metric.py, include/cpnative.h cp_online_metric_*): the properties of
the numpy definitions `fit_reference`, `apply_reference` and `stage_reference`, the point of the synthetic person, the tie rule
of `pick_shrink`, the stage's bookkeeping on a stand-in decoder, and the binding and host checks of the C entries."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import metric as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG = 10001
F = np.float32
ENTRIES = ["cp_online_metric_moments", "cp_online_metric_factor", "cp_online_metric_apply", "cp_online_metric_set",
           "cp_online_metric_reset", "cp_online_metric_push"]
R, I = M.REST, M.IGNORE
EYE = np.eye(16, dtype=F)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def person():
    """the synthetic person of 4 classes and 1,500 windows (8 repetitions), shared and left unchanged"""
    emb, exp = M.metric_recording(1500, 4, seed=0)
    emb.setflags(write=False)
    exp.setflags(write=False)
    return emb, exp, np.arange(4)


# ---------------------------------------------------------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_moments_are_a_scalar_loop_in_window_order(person):
    emb, exp, ids = person
    emb, exp = emb[:260], exp[:260]
    use = np.arange(260) % 5 != 0
    mom, cnt = M.moments_reference(emb, exp, ids, use)
    assert mom.shape == (4, 152) and mom.dtype == np.float64 and cnt.dtype == np.int64
    for c in range(4):
        n, s, p = 0, [np.float64(0.0)] * 16, {}
        for w in range(260):
            if exp[w] != c or not use[w]:
                continue
            n += 1
            e = [np.float64(v) for v in emb[w]]
            for d in range(16):
                s[d] = s[d] + e[d]
            for i in range(16):
                for j in range(i, 16):
                    p[i, j] = p.get((i, j), np.float64(0.0)) + e[i] * e[j]
        assert cnt[c] == n > 0
        assert same_bits(mom[c, :16], np.array(s))
        assert same_bits(mom[c, 16:], np.array([p[i, j] for i in range(16) for j in range(i, 16)]))


def test_the_factor_agrees_with_lapack_on_a_well_conditioned_scatter(person):
    """a sanity check, not a bit comparison: centred float64 scatter, np.linalg.cholesky and inv.  Measured on these inputs:
    5.1e-8 of the largest entry (the cast to f32 dominates: 2^-24 = 6.0e-8), condition numbers 13, 69 and 140; the bound is
    4 x that"""
    emb, exp, ids = person
    lams = (0.5, 0.1, 0.01)
    f = M.fit_reference(emb, exp, ids, lams, min_windows=10)
    assert f["valid"].all()
    x = emb.astype(np.float64)
    sw, n = np.zeros((16, 16)), 0
    for c in range(4):
        d = x[exp == c] - x[exp == c].mean(axis=0)
        sw += d.T @ d
        n += d.shape[0]
    sw /= n - 4
    s = np.trace(sw) / 16
    worst = 0.0
    for t, l in enumerate(lams):
        ref = np.linalg.inv(np.linalg.cholesky((1 - l) * sw / s + l * np.eye(16)))
        worst = max(worst, float(np.abs(f["A"][t].astype(np.float64) - ref).max() / np.abs(ref).max()))
        assert not np.triu(f["A"][t], 1).any() and (np.diag(f["A"][t]) > 0).all()
    print("deviation from LAPACK", worst)
    assert worst <= 4 * 5.1e-8


def test_shrink_one_is_the_identity_in_every_bit(person):
    emb, exp, ids = person
    f = M.fit_reference(emb, exp, ids, (1.0, 0.3, 1.0), min_windows=10)
    assert f["valid"].all() and same_bits(f["A"][0], EYE) and same_bits(f["A"][2], EYE) and not same_bits(f["A"][1], EYE)
    assert not np.signbit(f["A"][0]).any()                     # +0 everywhere off the diagonal, not -0


def test_scatters_that_do_not_factor_are_not_valid_and_leave_the_identity():
    u = np.full(16, 0.25, dtype=F)                             # a unit vector whose sums and products are exact
    same = np.tile(u, (32, 1))
    f = M.fit_reference(same, np.zeros(32, dtype=np.int64), [0], (0.0, 0.5, 1.0), min_windows=1)
    assert f["counts"].tolist() == [32] and not f["valid"].any()            # Sw = 0 exactly: s is not > 0
    assert all(same_bits(a, EYE) for a in f["A"])
    v = u.copy()
    v[0] = -0.25                                               # two exact points: a scatter of rank 1, exact in every entry
    two = np.stack([u, v] * 16)
    f = M.fit_reference(two, np.zeros(32, dtype=np.int64), [0], (0.0, 0.5, 1.0), min_windows=1)
    assert f["valid"].tolist() == [False, True, True] and same_bits(f["A"][0], EYE) and same_bits(f["A"][2], EYE)
    assert f["A"][1][0, 0] < f["A"][1][1, 1]                   # the loud axis is turned down
    # N - C < 1: two classes with one window each
    f = M.fit_reference(two[:2], np.array([0, 1]), [0, 1], (0.5, 1.0), min_windows=1)
    assert f["counts"].tolist() == [1, 1] and not f["valid"].any() and all(same_bits(a, EYE) for a in f["A"])
    # one more window and there is one degree of freedom
    f = M.fit_reference(two[:3], np.array([0, 0, 1]), [0, 1], (0.5,), min_windows=1)
    assert f["valid"].tolist() == [True]


def test_a_class_below_min_windows_is_left_out_of_the_pool(person):
    emb, exp, ids = person
    use = np.ones(1500, dtype=bool)
    use[np.nonzero(exp == 2)[0][7:]] = False                   # class 2 keeps seven windows
    with_it = M.fit_reference(emb, exp, ids, (0.5, 0.05), min_windows=10, use=use)
    without = M.fit_reference(emb, np.where(exp == 2, R, exp), ids, (0.5, 0.05), min_windows=10, use=use)
    assert with_it["counts"].tolist()[2] == 7 and without["counts"].tolist()[2] == 0
    assert same_bits(with_it["A"], without["A"]) and with_it["valid"].all()
    pooled = M.fit_reference(emb, exp, ids, (0.5, 0.05), min_windows=7, use=use)
    assert not same_bits(pooled["A"], with_it["A"])            # at min_windows = 7 it is in
    # a class alone gives what the full moments give for it
    alone = M.moments_reference(emb, np.where(exp == 3, exp, R), [3], use)
    full = M.moments_reference(emb, exp, ids, use)
    assert same_bits(alone[0][0], full[0][3]) and alone[1][0] == full[1][3]


def test_windows_that_do_not_train(person):
    emb, exp, ids = person
    emb, exp = emb.copy(), exp.copy()
    cue0 = np.nonzero(exp == 0)[0]
    emb[cue0[3], 4] = np.nan
    emb[cue0[7], 0] = np.inf
    emb[cue0[8], 15] = -np.inf
    emb[cue0[9]] = 0.0                                         # an all-zero window is finite: it trains
    exp[cue0[11:14]] = I
    use = np.ones(1500, dtype=bool)
    use[cue0[20:25]] = False
    f = M.fit_reference(emb, exp, np.array([0, 1, 2, 3, 9]), (0.2,), min_windows=10, use=use)
    assert f["counts"].tolist()[0] == cue0.size - 3 - 3 - 5 and f["counts"].tolist()[4] == 0 and np.isfinite(f["moments"]).all()
    drop = np.ones(1500, dtype=bool)
    drop[cue0[[3, 7, 8, 11, 12, 13, 20, 21, 22, 23, 24]]] = False
    g = M.fit_reference(emb[drop], exp[drop], np.array([0, 1, 2, 3, 9]), (0.2,), min_windows=10)
    assert same_bits(f["moments"], g["moments"]) and same_bits(f["counts"], g["counts"]) and same_bits(f["A"], g["A"])


def test_the_fit_refuses_what_it_cannot_take(person):
    emb, exp, ids = person
    emb, exp = emb[:200], exp[:200]
    for bad in (-0.1, 1.5, np.nan, [0.5, 2.0], [], [0.5] * 65):
        with pytest.raises(ValueError, match="shrink"):
            M.fit_reference(emb, exp, ids, bad)
    M.fit_reference(emb, exp, ids, [0.5] * 64)                 # 64 values are allowed
    for bad in (0, -3, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match="min_windows"):
            M.fit_reference(emb, exp, ids, min_windows=bad)
    for bad in ([1, 0, 2, 3], [0, 1, 1, 2], [-1, 0, 1, 2], list(range(65))):
        with pytest.raises(ValueError, match="ids"):
            M.fit_reference(emb, np.full(200, R), bad)
    with pytest.raises(ValueError, match="use"):
        M.fit_reference(emb, exp, ids, use=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="expected"):
        M.fit_reference(emb, np.where(exp == 0, 7, exp), ids)
    with pytest.raises(ValueError, match="embeddings"):
        M.fit_reference(emb[:, :8], exp, ids)
    with pytest.raises(ValueError, match="16, 16"):
        M.apply_reference(emb, np.eye(15, dtype=F))
    with pytest.raises(ValueError, match="rows"):
        M.stage_reference(emb, EYE, np.zeros((3, 16), F), ids)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="vote"):
            M.stage_reference(emb, EYE, np.ones((4, 16), F), ids, vote=bad)


# ---------------------------------------------------------------------------------------------------------------------------
# apply and the stage
# ---------------------------------------------------------------------------------------------------------------------------
def test_apply_with_the_identity_normalises_and_keeps_what_is_not_finite_not_finite(person):
    emb, _, _ = person
    x = (emb[:300] * F(3.5)).astype(F)
    x[5, 2], x[6, 15], x[7] = np.nan, np.inf, 0.0
    with np.errstate(all="ignore"):
        ss = np.zeros(300, dtype=F)
        for d in range(16):
            ss = ss + x[:, d] * x[:, d]
        want = x / np.sqrt(ss)[:, None]
    got = M.apply_reference(x, EYE)
    ok = np.isfinite(x).all(axis=1) & (ss > 0)
    assert ok.sum() == 297 and same_bits(got[ok], want[ok]) and got.dtype == F
    assert not np.isfinite(got[~ok]).all(axis=1).any()
    # the upper triangle is not read
    a = EYE.copy()
    a[0, 5] = 7.0
    assert same_bits(M.apply_reference(x[ok], a), got[ok])


def test_the_stage_is_the_holdout_tail_on_the_whitened_embeddings(person):
    emb, exp, ids = person
    f = M.fit_reference(emb, exp, ids, (0.1,), min_windows=10)
    e2 = M.apply_reference(emb, f["A"][0])
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((4, 16)) * 2).astype(F)        # not unit: both sides normalise
    e = emb.copy()
    e[40, 3] = np.nan                                          # a window that predicts none and takes a place in the ring
    e2 = M.apply_reference(e, f["A"][0])
    for vote in (1, 9, 25):
        st = M.stage_reference(e, f["A"][0], rows, ids, vote=vote)
        assert same_bits(st["embeddings"], e2)
        ho = H.holdout_reference(e2, exp, ids, np.zeros(1500, dtype=np.int32), rows,
                                 [dict(train=0, eval=1, mix=1.0, min_windows=1)], vote=vote, return_sequences=True)
        assert same_bits(ho["pred"][0], st["pred"]) and same_bits(ho["voted"][0], st["voted"])
        assert st["pred"][40] == -1 and same_bits(st["logits"], H._logits(e2, ho["unit"][0]))
    # ties go to the smallest id, -0 equals +0
    two = M.stage_reference(emb[:5], EYE, np.stack([emb[0], emb[0], -emb[0]]), [3, 5, 8], vote=2)
    assert two["pred"][0] == 3 and set(two["pred"].tolist()) <= {3, 8}


def test_whitening_decodes_held_out_repetitions_that_the_plain_cosine_loses(person):
    """leave one repetition out, eight times, on the definitions alone: 683 voted hits of 1,200 cue windows with the plain
    cosine, 1,033 with the picked shrink value 0.1"""
    emb, exp, ids = person
    r = M.pick_shrink_reference(emb, exp, ids, (1.0,) + M.SHRINKS, min_windows=10)
    assert r["n_rep"] == 8 and (r["n_cue"] == 1200).all() and r["baseline"][1] == 1200
    assert r["voted_hit"][0] == r["baseline"][0]               # shrink 1 is the plain cosine
    print("plain", r["baseline"], "whitened", r["voted_hit"].tolist(), "picked", r["shrink"])
    assert r["shrink"] < 1.0 and r["voted_hit"][r["best"]] > r["baseline"][0] + 200
    assert r["baseline"][0] == 683 and int(r["voted_hit"][r["best"]]) == 1033 and r["shrink"] == 0.1


def test_pick_shrink_takes_the_larger_shrink_value_among_equals(person):
    emb, exp, ids = person
    hits = {0.5: 7, 0.2: 9, 0.1: 9, 0.05: 3}
    valid = {0.5: True, 0.2: True, 0.1: True, 0.05: True}

    def run(lams):
        fit = lambda use, lam, minw: (list(lam), [valid[float(l)] for l in lam])
        score = lambda e, rep, pr, plans, v: (5, 10) if isinstance(e, np.ndarray) else (hits[float(e)], 10)
        return M._pick(fit, lambda a: float(a), score, emb, exp, ids, lams, 2, 25, 10, None)

    r = run((0.05, 0.1, 0.2, 0.5))
    assert r["best"] == 2 and r["shrink"] == 0.2 and r["voted_hit"].tolist() == [6, 18, 18, 14] and r["baseline"] == (10, 20)
    assert run((0.2, 0.1))["best"] == 0 and run((0.1, 0.2))["best"] == 1 and (r["n_cue"] == 20).all() and r["n_rep"] == 2
    valid[0.2] = False                                         # a value that is not valid in a fold never wins
    r = run((0.05, 0.1, 0.2, 0.5))
    assert r["best"] == 1 and r["voted_hit"].tolist() == [6, 18, -1, 14]
    valid.update({0.5: False, 0.1: False, 0.05: False})
    assert run((0.05, 0.1))["best"] is None and run((0.05, 0.1))["shrink"] is None
    with pytest.raises(ValueError, match="two repetitions"):
        M.pick_shrink_reference(emb[:60], exp[:60], ids, (0.5,))


def test_metric_recording_is_repeatable_and_has_one_loud_axis():
    a, b = M.metric_recording(700, 3, seed=4), M.metric_recording(700, 3, seed=4)
    assert all(same_bits(x, y) for x, y in zip(a, b)) and a[0].dtype == F and a[0].shape == (700, 16)
    emb, exp = a
    assert np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-6) and set(exp.tolist()) == {R, 0, 1, 2}
    x = emb.astype(np.float64)
    sw = sum((x[exp == c] - x[exp == c].mean(axis=0)).T @ (x[exp == c] - x[exp == c].mean(axis=0)) for c in range(3))
    ev = np.linalg.eigvalsh(sw)
    # one direction carries the within-class spread; the normalisation bends part of it into the common direction of the
    # centres, which is the second eigenvalue, and the quiet noise is far below both
    # (by construction 0.6^2 * 2 against 0.05^2 per axis, 288 : 1, before the normalisation compresses the loud axis)
    assert ev[-1] > 5 * ev[-2] and ev[-1] > 50 * ev[-3]
    with pytest.raises(ValueError):
        M.metric_recording(100, 65)


# ---------------------------------------------------------------------------------------------------------------------------
# the stage's bookkeeping on a stand-in decoder
# ---------------------------------------------------------------------------------------------------------------------------
class Fake:
    class_ids, n_seen, vote, ws, device = None, 0, 25, None, None

    def push(self, *a, **k):
        raise AssertionError


def test_the_stage_keeps_its_own_ids_and_follows_the_decoder_without_a_device(person):
    emb, exp, ids = person
    met = M.Metric.of(M.fit_reference(emb, exp, ids, (0.0, 0.1, 1.0), min_windows=10))
    assert met.valid.tolist() == [True, True, True] and met.A.shape == (3, 16, 16)
    rows = np.ones((4, 16), dtype=F)
    dec = Fake()
    dec.class_ids = np.array([0, 1, 2, 3, 4, 5], dtype=np.int32)
    stage = M.MetricRows(dec)
    assert stage.class_ids is dec.class_ids and stage.vote == 25 and stage.n_seen == 0 and not stage.multi   # it sits out
    stage.set(met, rows, t=1)
    first = stage.class_ids
    assert first.tolist() == [0, 1, 2, 3] and stage.class_ids is first
    stage.set(met, rows[:2], ids=[7, 9], t=2)
    assert stage.class_ids.tolist() == [7, 9]
    assert met.install(dec, rows, stage=stage) is stage and stage.class_ids.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="rows"):
        stage.set(met, rows[:3])
    with pytest.raises(ValueError, match="rows"):
        stage.set(met, None)
    with pytest.raises(ValueError, match="ids"):
        stage.set(met, rows[:2], ids=[9, 7])
    with pytest.raises(IndexError):
        stage.set(met, rows, t=3)
    with pytest.raises(TypeError):
        stage.set(object(), rows)
    with pytest.raises(TypeError):
        M.MetricRows(object())
    with pytest.raises(TypeError, match="push_packed"):
        stage.push_packed(None, None)
    with pytest.raises(ValueError, match="stage="):
        met.install(Fake(), rows, stage=stage)
    # an invalid metric is a ValueError, wherever it is asked for
    bad = M.Metric.of(M.fit_reference(emb[:40], exp[:40], ids, (0.5,), min_windows=100))
    assert not bad.valid.any()
    for call in (lambda: M.MetricRows(dec, bad, rows), lambda: bad.apply(emb), lambda: bad.install(dec, rows)):
        with pytest.raises(ValueError, match="no valid metric"):
            call()
    assert same_bits(met.apply(emb, 1), M.apply_reference(emb, met.A[1]))
    dec.n_seen = 40
    with pytest.raises(Exception, match="behind the metric stage"):
        stage.push(None)
    # a multi-stream decoder: each stream its own, the others sit out with the decoder's ids
    multi = Fake()
    multi.class_ids, multi.n_seen = [None, np.array([4, 5, 12]), np.array([1, 2])], np.zeros(3, dtype=np.int64)
    with pytest.raises(ValueError, match="stream"):
        M.MetricRows(multi, met, rows)
    st = M.MetricRows(multi, met, rows, stream=2)
    assert st.multi and st.class_ids[0] is None and st.class_ids[1] is multi.class_ids[1] and st.class_ids[2].tolist() == [0, 1, 2, 3]
    assert met.install(multi, rows[:1], ids=[6], stream=0, stage=st) is st and st.class_ids[0].tolist() == [6]
    with pytest.raises(IndexError):
        st.set(met, rows, stream=3)


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
    assert hasattr(raw, "cp_online_metric_workspace_bytes") and "cp_online_metric_workspace_bytes" in _lib.SYMBOLS
    for name in ("CP_ONLINE_METRIC_MOMENTS", "CP_ONLINE_METRIC_MAX_SHRINKS", "CP_ONLINE_METRIC_RESET_RING", "CP_ONLINE_METRIC_RESET_ALL"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(_lib, name), name
    assert M.MOMENTS == 152 and M.MAX_SHRINKS == 64
    one = lib.cp_online_metric_workspace_bytes(1)
    assert one == (M._OM_WORDS * 4 + 255) // 256 * 256 == lib.cp_online_metric_workspace_bytes(0)
    assert lib.cp_online_metric_workspace_bytes(256) == 256 * M._OM_WORDS * 4


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory for every pointer: each refusal returns before a launch, which on a machine without a GPU would fail otherwise"""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    lam = (ctypes.c_double * 64)(*([0.5] * 64))

    def err(rc, entry, what):
        assert rc == ERR_ARG, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    name = "cp_online_metric_moments"
    mo = lambda emb=p, m=8, k=3, slot=p, use=None, mom=p, cnt=p: lib.cp_online_metric_moments(emb, m, k, slot, use, mom, cnt, None)
    for m in (0, -1, 2 ** 31):
        err(mo(m=m), name, "n_rows")
    for k in (0, 65, -1):
        err(mo(k=k), name, "n_classes")
    for arg in ("emb", "slot", "mom", "cnt"):
        err(mo(**{arg: None}), name, "required")
    for arg in ("slot", "mom", "cnt"):
        err(mo(**{arg: p + 2}), name, "misaligned")
    err(mo(mom=p + 4), name, "misaligned")
    err(mo(emb=p + 8), name, "16-byte")

    name = "cp_online_metric_factor"
    fa = lambda mom=p, cnt=p, k=3, minw=5, sh=lam, n=5, a=p, valid=p: lib.cp_online_metric_factor(mom, cnt, k, minw, sh, n, a, valid, None)
    for k in (0, 65, -1):
        err(fa(k=k), name, "n_classes")
    for mw in (0, -1):
        err(fa(minw=mw), name, "min_windows")
    for n in (0, 65, -1):
        err(fa(n=n), name, "n_shrinks")
    for arg in ("mom", "cnt", "sh", "a", "valid"):
        err(fa(**{arg: None}), name, "required")
    for arg in ("mom", "cnt", "a"):
        err(fa(**{arg: p + 2}), name, "misaligned")
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        err(fa(sh=(ctypes.c_double * 5)(0.5, 0.0, 1.0, bad, 0.1)), name, "[0, 1]")

    name = "cp_online_metric_apply"
    ap = lambda emb=p, m=8, a=p, out=p + 4096: lib.cp_online_metric_apply(emb, m, a, out, None)
    for m in (0, -1, 2 ** 31):
        err(ap(m=m), name, "n_rows")
    for arg in ("emb", "a", "out"):
        err(ap(**{arg: None}), name, "required")
    err(ap(emb=p + 8), name, "16-byte")
    err(ap(out=p + 8), name, "16-byte")
    err(ap(a=p + 2), name, "misaligned")

    S = 3
    need = lib.cp_online_metric_workspace_bytes(S)
    ids = (ctypes.c_int32 * 3)(4, 5, 8)
    se, rs, pu = "cp_online_metric_set", "cp_online_metric_reset", "cp_online_metric_push"

    def entries(vote=25, n_streams=S, w=p, nbytes=need):
        return ((se, lambda: lib.cp_online_metric_set(vote, n_streams, w, nbytes, 0, p, p, ids, 3, None)),
                (rs, lambda: lib.cp_online_metric_reset(vote, n_streams, w, nbytes, -1, 0, None)),
                (pu, lambda: lib.cp_online_metric_push(vote, n_streams, w, nbytes, p, p, p, 1, p, p, None, 0, None)))

    for vote in (0, 257, -1):
        for entry, call in entries(vote=vote):
            err(call(), entry, "vote")
    for n in (0, 257):
        for entry, call in entries(n_streams=n):
            err(call(), entry, "n_streams")
    for entry, call in entries(w=None):
        err(call(), entry, "workspace")
    for entry, call in entries(w=p + 64):
        err(call(), entry, "256-byte")
    for nbytes in (need - 256, need + 256, 0):                 # exactly the workspace size
        for entry, call in entries(nbytes=nbytes):
            err(call(), entry, "ws_bytes")
    st = lambda index=0, a=p, rows=p, i=ids, k=3: lib.cp_online_metric_set(25, S, p, need, index, a, rows, i, k, None)
    for k in (0, 65):
        err(st(k=k), se, "classes")
    err(st(i=None), se, "classes")
    err(st(a=None, rows=None), se, "A or rows")
    for index in (S, -1):
        err(st(index=index), se, "stream index")
    for bad in ((5, 4, 8), (4, 4, 8), (-1, 4, 8), (4, 5, 2 ** 31 - 1)):
        err(st(i=(ctypes.c_int32 * 3)(*bad)), se, "ascending")
    for arg in ("a", "rows"):
        err(st(**{arg: p + 2}), se, "misaligned")
    for index in (S, -2):
        err(lib.cp_online_metric_reset(25, S, p, need, index, 0, None), rs, "stream index")
    for what in (-1, 2):
        err(lib.cp_online_metric_reset(25, S, p, need, 0, what, None), rs, "what")
    push = lambda emb=p, row0=p, m=p, total=1, pred=p, voted=p, lg=None, ldl=0: \
        lib.cp_online_metric_push(25, S, p, need, emb, row0, m, total, pred, voted, lg, ldl, None)
    for total in (-1, 65537):
        err(push(total=total), pu, "total_rows")
    err(push(lg=p, ldl=0), pu, "ldl")
    for arg in ("emb", "row0", "m", "pred", "voted"):
        err(push(**{arg: None}), pu, "required")
    for arg in ("row0", "m", "pred", "voted"):
        err(push(**{arg: p + 2}), pu, "misaligned")
    err(push(lg=p + 2, ldl=4), pu, "misaligned")
    err(push(emb=p + 8), pu, "16-byte")
    assert lib.cp_online_metric_push(25, S, p, need, None, None, None, 0, None, None, None, 0, None) == 0     # nothing to do


def test_wrappers_check_before_they_touch_a_device_and_are_exported_lazily(person):
    import contrastiveprosthetics_amd as pkg
    assert pkg.fit_metric is M.fit_metric and pkg.Metric is M.Metric and pkg.MetricRows is M.MetricRows
    assert pkg.pick_shrink is M.pick_shrink and pkg.metric_enrolment is M.metric_enrolment and pkg.metric_recording is M.metric_recording
    emb, exp, ids = person
    for kw, what in ((dict(shrink=1.5), "shrink"), (dict(shrink=[0.5] * 65), "shrink"), (dict(min_windows=0), "min_windows"),
                     (dict(ids=[1, 0, 2, 3]), "ascending"), (dict(ids=list(range(65))), "ids")):
        args = dict(embeddings=emb, expected=exp, ids=ids)
        args.update(kw)
        with pytest.raises(ValueError, match=what):            # (before the embeddings are looked at)
            M.fit_metric(**args)
    with pytest.raises(ValueError, match="embeddings"):
        M.fit_metric(emb, exp, ids)                            # numpy, not a GPU tensor
    with pytest.raises(ValueError, match="embeddings"):
        M.pick_shrink(emb, exp, ids)
