"""Held-out enrolment scoring without a GPU (contrastiveprosthetics_amd/holdout.py, include/cpnative.h cp_online_holdout_*):
repetitions and plans, the properties of the numpy definition `holdout_reference` on a seeded synthetic recording, and the
binding and host checks of the four C entries."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd.track import track_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG = 10001
F = np.float32
ENTRIES = ["cp_online_holdout_sums", "cp_online_holdout_tables", "cp_online_holdout_score", "cp_online_holdout_logits"]
R, I = H.REST, H.IGNORE


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# repetitions, plans, folds
# ---------------------------------------------------------------------------------------------------------------------------
def test_repetitions_count_per_class_and_fill_the_gaps_forwards():
    #             0  1  2  3  4  5  6  7  8  9 10 11 12 13 14
    exp = np.array([R, 5, 5, R, 7, 7, I, 5, R, R, 5, 5, 7, R, I])
    rep, n = H.repetitions(exp)
    # class 5 has three segments (rows 1-2, 7, 10-11), class 7 two (4-5, 12); a gap takes the next segment's repetition, the tail
    # behind the last segment that segment's
    assert n == 3 and rep.dtype == np.int32
    assert rep.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 1, 1, 1]


def test_repetitions_fold_and_refuse_more_than_32():
    exp = np.concatenate([[c, R] for _ in range(5) for c in (3, 9)])          # 5 repetitions of two classes, a rest behind each
    rep, n = H.repetitions(exp)
    want = [min((i + 1) // 4, 4) for i in range(20)]          # the rest behind a repetition's last cue goes with the next one
    assert n == 5 and rep.tolist() == want
    rep, n = H.repetitions(exp, folds=2)
    assert n == 2 and rep.tolist() == [r % 2 for r in want]
    many = np.concatenate([[4, R]] * 33)
    with pytest.raises(ValueError, match="folds="):
        H.repetitions(many)
    rep, n = H.repetitions(many, folds=32)
    assert n == 32 and rep[-2:].tolist() == [0, 0] and rep[61:64].tolist() == [31, 31, 0]
    for bad in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="folds"):
            H.repetitions(exp, folds=bad)


def test_repetitions_without_segments_and_trailing_rest():
    rep, n = H.repetitions(np.array([R, I, R, R]))
    assert n == 0 and rep.tolist() == [-1] * 4
    rep, n = H.repetitions(np.zeros(0, dtype=np.int64))
    assert n == 0 and rep.shape == (0,)
    rep, n = H.repetitions(np.array([2, 2, R, 2, R, R, R]))
    assert n == 2 and rep.tolist() == [0, 0, 1, 1, 1, 1, 1]


def test_plan_builders_sizes_and_masks():
    loo = H.leave_one_out(6, mix=0.5, min_windows=3)
    assert len(loo) == 6
    for h, p in enumerate(loo):
        assert p == dict(train=0b111111 & ~(1 << h), eval=1 << h, mix=0.5, min_windows=3)
    assert H.leave_one_out(1) == [dict(train=0, eval=1, mix=1.0, min_windows=25)]
    assert H.leave_one_out(32)[31]["train"] == 2 ** 31 - 1 and H.leave_one_out(32)[0]["train"] == 2 ** 32 - 2
    lc = H.learning_curve(6)
    assert len(lc) == 30
    for h in range(6):
        for n in range(1, 6):
            p = lc[h * 5 + n - 1]
            assert p["eval"] == 1 << h and bin(p["train"]).count("1") == n and not p["train"] & p["eval"]
            assert p["train"] == sum(1 << ((h + j) % 6) for j in range(1, n + 1))
        assert lc[h * 5 + 4]["train"] == loo[h]["train"]
    assert H.learning_curve(1) == []
    grid = H.plan_grid(loo, mix=[0.0, 1.0], min_windows=[1, 10, 25])
    assert len(grid) == 36
    assert [(g["eval"], g["mix"], g["min_windows"]) for g in grid[:7]] == \
        [(1, 0.0, 1), (1, 0.0, 10), (1, 0.0, 25), (1, 1.0, 1), (1, 1.0, 10), (1, 1.0, 25), (2, 0.0, 1)]
    assert H.plan_grid(loo) == loo and H.plan_grid(loo)[0] is not loo[0]
    for bad in (0, 33, True):
        with pytest.raises(ValueError):
            H.leave_one_out(bad)


def test_assign_folds_on_leave_one_out_covers_every_window_with_a_repetition_once():
    rng = np.random.default_rng(0)
    rep = rng.integers(-1, 6, 500).astype(np.int32)
    loo = H.leave_one_out(6)
    a = H.assign_folds(rep, loo)
    assert a.dtype == np.int32 and (a[rep < 0] == -1).all() and (a[rep >= 0] == rep[rep >= 0]).all()
    held = np.array([[bool(p["eval"] >> r & 1) for r in rep.clip(0)] for p in loo]) & (rep >= 0)
    assert (held.sum(axis=0) == (rep >= 0)).all()
    lc = H.learning_curve(6)
    assert (H.assign_folds(rep, lc)[rep >= 0] == 5 * rep[rep >= 0]).all()                     # the first: one training repetition
    assert (H.assign_folds(rep, lc, most_trained=True)[rep >= 0] == 5 * rep[rep >= 0] + 4).all()
    refused = [dict(loo[0], mix=2.0)] + loo[1:]
    assert (H.assign_folds(rep, refused)[rep == 0] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------
def recording(k=5, reps=3, **kw):
    ids = np.arange(k) * 3 + 2                                         # class ids that are not their slots
    emb, exp, prior = H.cued_recording(k, reps, segment=12, rest=4, seed=2, ids=ids, **kw)
    return emb, exp, prior, ids


@pytest.mark.parametrize("vote", [1, 5, 25])
def test_training_and_scoring_on_everything_is_the_static_decoder_on_the_unit_rows(vote):
    emb, exp, prior, ids = recording()
    rep, n = H.repetitions(exp)
    assert n == 3 and (rep >= 0).all()
    plan = dict(train=0b111, eval=0b111, mix=0.7, min_windows=5)
    ref = H.holdout_reference(emb, exp, ids, rep, prior, [plan], vote=vote, return_sequences=True)
    trk = track_reference(emb, ref["unit"][0], ids, rate=0.0, vote=vote)
    assert np.array_equal(ref["pred"][0], trk["pred"]) and np.array_equal(ref["voted"][0], trk["voted"])
    logits = H.holdout_logits_reference(emb, ref["unit"], np.zeros(emb.shape[0], dtype=np.int32))
    assert same_bits(logits, trk["logits"])
    cue = exp >= 0
    assert ref["n_cue"][0] == cue.sum() and ref["n_rest"][0] == (exp == R).sum() and ref["n_train"][0] == cue.sum()
    assert ref["pred_hit"][0] == (cue & (trk["pred"] == exp)).sum() and ref["voted_hit"][0] == (cue & (trk["voted"] == exp)).sum()
    assert ref["n_enrolled"][0] == 5 and ref["confusion"][0].sum() == cue.sum()
    assert np.trace(ref["confusion"][0]) == ref["pred_hit"][0] and np.trace(ref["voted_confusion"][0]) == ref["voted_hit"][0]
    k = int(np.argmin(ref["voted_confusion"][0].diagonal() / ref["voted_confusion"][0].sum(axis=1)))
    assert ref["worst_class"][0] == ids[k] and ref["worst_n"][0] == 36
    assert ref["worst_hit"][0] == ref["voted_confusion"][0][k, k]


def test_the_sums_are_the_enrolment_accumulator_and_the_rows_its_blend():
    emb, exp, prior, ids = recording()
    rep, _ = H.repetitions(exp)
    ref = H.holdout_reference(emb, exp, ids, rep, prior, H.leave_one_out(3, mix=0.6, min_windows=1))
    for t in range(3):
        for c in range(5):
            acc, n = np.zeros(16), 0
            for i in range(emb.shape[0]):
                if exp[i] == ids[c] and rep[i] != t:
                    acc = acc + emb[i].astype(np.float64)
                    n += 1
            assert same_bits(ref["sums"][t, c], acc) and ref["counts"][t, c] == n == 24
            length = np.float64(np.sqrt(np.sum(prior[c] * prior[c], dtype=F)))
            row = (0.4 * prior[c].astype(np.float64) + 0.6 * (length * (acc / np.sqrt(np.sum(acc * acc))))).astype(F)
            assert np.allclose(ref["rows"][t, c], row, rtol=0, atol=1e-7)
            assert abs(float(np.linalg.norm(ref["unit"][t, c].astype(np.float64))) - 1.0) < 1e-6
    # (the rest behind a repetition's last cue belongs to the next repetition, the rest at the end to the last)
    assert (ref["n_train"] == 120).all() and (ref["n_cue"] == 60).all() and ref["n_rest"].tolist() == [16, 20, 24]
    # a held-out repetition is harder than the one the rows were made from
    own = H.holdout_reference(emb, exp, ids, rep, prior, [dict(train=0b111, eval=1 << t, mix=0.6, min_windows=1) for t in range(3)])
    assert own["pred_hit"].sum() >= ref["pred_hit"].sum()


def test_a_plan_that_trains_nothing_and_a_class_below_min_windows_keep_the_prior_bit_for_bit():
    emb, exp, prior, ids = recording()
    rep, _ = H.repetitions(exp)
    ref = H.holdout_reference(emb, exp, ids, rep, prior, [dict(train=0, eval=0b111, mix=1.0, min_windows=1),
                                                          dict(train=0b001, eval=0b110, mix=1.0, min_windows=12),
                                                          dict(train=0b001, eval=0b110, mix=1.0, min_windows=13),
                                                          dict(train=0b111, eval=0b111, mix=0.0, min_windows=1)])
    assert same_bits(ref["rows"][0], prior) and ref["n_train"][0] == 0 and ref["n_enrolled"][0] == 0
    assert ref["n_enrolled"][1] == 5 and not (ref["rows"][1] == prior).all(axis=1).any()
    assert ref["n_enrolled"][2] == 0 and same_bits(ref["rows"][2], prior) and ref["n_train"][2] == 60
    assert same_bits(ref["rows"][3], prior)                                    # mix = 0 reproduces the table
    # one class short of windows: its cue in repetition 0 is IGNORE except for three windows
    exp2 = exp.copy()
    first = np.nonzero((exp == ids[2]) & (rep == 0))[0]
    exp2[first[3:]] = I
    ref2 = H.holdout_reference(emb, exp2, ids, rep, prior, [dict(train=0b001, eval=0b110, mix=1.0, min_windows=4)])
    assert ref2["n_enrolled"][0] == 4 and same_bits(ref2["rows"][0][2], prior[2])
    assert not (ref2["rows"][0][[0, 1, 3, 4]] == prior[[0, 1, 3, 4]]).all(axis=1).any()


def test_refused_plans_score_minus_one_and_write_nothing():
    emb, exp, prior, ids = recording()
    rep, _ = H.repetitions(exp)
    good = dict(train=0b110, eval=0b001, mix=1.0, min_windows=5)
    bad = [dict(good, mix=-0.01), dict(good, mix=1.5), dict(good, mix=float("nan")), dict(good, mix=float("inf")),
           dict(good, min_windows=0), dict(good, min_windows=-3), dict(good, train=1 << 32), dict(good, eval=1 << 40),
           dict(good, train=-1)]
    ref = H.holdout_reference(emb, exp, ids, rep, prior, [good] + bad + [good], return_sequences=True)
    for key in H.HOLDOUT_SCORE_KEYS:
        assert (ref[key][1:-1] == -1).all() and ref[key][0] == ref[key][-1] and ref[key][0] >= 0, key
    assert not ref["rows"][1:-1].any() and not ref["unit"][1:-1].any() and not ref["confusion"][1:-1].any()
    assert (ref["pred"][1:-1] == H.NOT_EVALUATED).all() and (ref["voted"][1:-1] == H.NOT_EVALUATED).all()
    assert same_bits(ref["rows"][0], ref["rows"][-1]) and np.array_equal(ref["pred"][0], ref["pred"][-1])
    assert ((ref["pred"][0] == H.NOT_EVALUATED) == (rep != 0)).all()
    # what is not a plan at all is an error, as are inputs that do not fit
    for wrong in ([], [good] * 4097, [dict(train=1, eval=1, mix=1.0, min_windows=1.5)], [dict(train=1.0, eval=1)], [dict(train=1)],
                  [dict(good, extra=1)], ["plan"]):
        with pytest.raises(ValueError):
            H.holdout_reference(emb, exp, ids, rep, prior, wrong)
    zero = prior.copy()
    zero[1] = 0
    with pytest.raises(ValueError, match="prior"):
        H.holdout_reference(emb, exp, ids, rep, zero, [good])
    with pytest.raises(ValueError, match="folds="):
        H.holdout_reference(emb, exp, ids, rep + 30, prior, [good])
    with pytest.raises(ValueError, match="vote"):
        H.holdout_reference(emb, exp, ids, rep, prior, [good], vote=257)


def test_rows_that_are_not_numbers_predict_nothing_and_take_a_place_in_the_ring():
    emb, exp, prior, ids = recording()
    rep, _ = H.repetitions(exp)
    ev = np.nonzero(rep == 0)[0]
    emb = emb.copy()
    emb[ev[5], 3] = np.nan
    emb[ev[6], 0] = np.inf
    emb[ev[:3]] = np.nan                                                        # the ring starts with nothing but "none"
    plan = dict(train=0b110, eval=0b001, mix=1.0, min_windows=5)
    ref = H.holdout_reference(emb, exp, ids, rep, prior, [plan], vote=3, return_sequences=True)
    assert (ref["pred"][0][ev[[0, 1, 2, 5, 6]]] == -1).all() and (ref["voted"][0][ev[:3]] == -1).all()
    assert ref["voted"][0][ev[3]] == ref["pred"][0][ev[3]] >= 0
    assert ref["voted"][0][ev[6]] == ref["pred"][0][ev[4]]                      # ring: 4, none, none
    assert ref["n_cue"][0] == 60 and ref["confusion"][0].sum() == 60 - 5
    logits = H.holdout_logits_reference(emb, ref["unit"], np.where(rep == 0, 0, -1))
    assert np.isnan(logits[rep != 0]).all() and np.isnan(logits[ev[0]]).all() and np.isfinite(logits[ev[7]]).all()
    # NaN among the training windows: |S| > 0 does not hold, so the class keeps its prior row, as in enroll; the others enrol
    emb2 = H.cued_recording(5, 3, segment=12, rest=4, seed=2, ids=ids)[0]
    bad = np.nonzero((exp == ids[1]) & (rep == 1))[0][0]
    emb2[bad, 7] = np.nan
    ref2 = H.holdout_reference(emb2, exp, ids, rep, prior, [plan])
    assert np.isnan(ref2["sums"][0][1][7]) and same_bits(ref2["rows"][0][1], prior[1]) and np.isfinite(ref2["rows"][0]).all()
    assert not (ref2["rows"][0][[0, 2, 3, 4]] == prior[[0, 2, 3, 4]]).all(axis=1).any() and ref2["n_enrolled"][0] == 5


# ---------------------------------------------------------------------------------------------------------------------------
# the binding and the host checks of the entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_struct_constants_and_symbols_match_the_header(lib):
    from contrastiveprosthetics_amd import _lib
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in ENTRIES:
        assert hasattr(raw, n) and n in _lib.SYMBOLS, n
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert m and len(m.group(1).split(",")) == len(_lib.SYMBOLS[n][1]), n
    body = hdr[hdr.index("typedef struct cp_online_holdout_plan {"):hdr.index("} cp_online_holdout_plan;")]
    assert re.findall(r"\b(?:uint32_t|int32_t|double)\s+(\w+);", body) == [f[0] for f in _lib.cp_online_holdout_plan._fields_]
    assert ctypes.sizeof(_lib.cp_online_holdout_plan) == 24 == H._PLAN_DTYPE.itemsize
    assert _lib.cp_online_holdout_plan.mix.offset == 16 == H._PLAN_DTYPE.fields["mix"][1]
    assert _lib.cp_online_holdout_plan.sums_index.offset == 8 == H._PLAN_DTYPE.fields["sums_index"][1]
    for name in ("CP_ONLINE_HOLDOUT_SCORES", "CP_ONLINE_HOLDOUT_MAX_PLANS", "CP_ONLINE_HOLDOUT_MAX_REPS"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(_lib, name), name
    assert len(H.HOLDOUT_SCORE_KEYS) == _lib.CP_ONLINE_HOLDOUT_SCORES == 9 and H.MAX_PLANS == 4096 and H.MAX_REPS == 32


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory for every pointer: each refusal returns before a launch, which on a machine without a GPU would fail otherwise"""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    M, K, T = 8, 3, 2

    def err(rc, entry, what):
        assert rc == ERR_ARG, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    def sums(emb=p, m=M, k=K, slot=p, rep=p, masks=p, n=T, out=p):
        return lib.cp_online_holdout_sums(emb, m, k, slot, rep, masks, n, out, None)

    def tables(s=p, n=T, k=K, prior=p, plans=p, t=T, rows=p, unit=p):
        return lib.cp_online_holdout_tables(s, n, k, prior, plans, t, rows, unit, None)

    def score(emb=p, m=M, k=K, slot=p, rep=p, unit=p, plans=p, t=T, vote=25, sc=p, c=None, vc=None, pr=None, vo=None):
        return lib.cp_online_holdout_score(emb, m, k, slot, rep, unit, plans, t, vote, sc, c, vc, pr, vo, None)

    def logits(emb=p, m=M, k=K, unit=p, t=T, assign=p, out=p, ldl=K):
        return lib.cp_online_holdout_logits(emb, m, k, unit, t, assign, out, ldl, None)

    for entry, fn in (("cp_online_holdout_sums", sums), ("cp_online_holdout_score", score), ("cp_online_holdout_logits", logits)):
        for m in (0, -1, 2 ** 31):
            err(fn(m=m), entry, "n_rows")
        for k in (0, 65, -1):
            err(fn(k=k), entry, "n_classes")
        err(fn(emb=None), entry, "required")
    for k in (0, 65):
        err(tables(k=k), "cp_online_holdout_tables", "n_classes")
    for n in (0, 4097, -1):
        err(sums(n=n), "cp_online_holdout_sums", "n_masks")
        err(tables(n=n), "cp_online_holdout_tables", "n_masks")
        err(tables(t=n), "cp_online_holdout_tables", "n_plans")
        err(score(t=n), "cp_online_holdout_score", "n_plans")
        err(logits(t=n), "cp_online_holdout_logits", "n_plans")
    for name in ("slot", "rep", "masks", "out"):
        err(sums(**{name: None}), "cp_online_holdout_sums", "required")
        err(sums(**{name: p + 2}), "cp_online_holdout_sums", "misaligned")
    err(sums(out=p + 4), "cp_online_holdout_sums", "misaligned")
    err(sums(emb=p + 8), "cp_online_holdout_sums", "16-byte")
    for name in ("s", "prior", "plans", "rows", "unit"):
        err(tables(**{name: None}), "cp_online_holdout_tables", "required")
        err(tables(**{name: p + 2}), "cp_online_holdout_tables", "misaligned")
    err(tables(s=p + 4), "cp_online_holdout_tables", "misaligned")
    err(tables(plans=p + 4), "cp_online_holdout_tables", "misaligned")
    err(tables(unit=p + 8), "cp_online_holdout_tables", "misaligned")
    for name in ("slot", "rep", "unit", "plans", "sc"):
        err(score(**{name: None}), "cp_online_holdout_score", "required")
    for name in ("slot", "rep", "plans", "sc", "c", "vc", "pr", "vo"):
        err(score(**{name: p + 2}), "cp_online_holdout_score", "misaligned")
    err(score(emb=p + 8), "cp_online_holdout_score", "16-byte")
    err(score(unit=p + 4), "cp_online_holdout_score", "16-byte")
    err(score(sc=p + 4), "cp_online_holdout_score", "misaligned")
    for v in (0, 257, -1):
        err(score(vote=v), "cp_online_holdout_score", "vote")
    for name in ("unit", "assign", "out"):
        err(logits(**{name: None}), "cp_online_holdout_logits", "required")
        err(logits(**{name: p + 2}), "cp_online_holdout_logits", "misaligned")
    err(logits(ldl=K - 1), "cp_online_holdout_logits", "ldl")


def test_wrappers_check_before_they_touch_a_device_and_are_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    assert pkg.score_enrolment is H.score_enrolment and pkg.score_plans is H.score_plans and pkg.holdout_reference is H.holdout_reference
    assert pkg.HOLDOUT_SCORE_KEYS == H.HOLDOUT_SCORE_KEYS
    emb, exp, prior, ids = recording()
    rep, _ = H.repetitions(exp)
    with pytest.raises(ValueError, match="embeddings"):
        H.score_plans(emb, exp, ids, rep, prior, H.leave_one_out(3))           # numpy: not on a GPU
    import torch
    with pytest.raises(ValueError, match="GPU"):
        H.score_plans(torch.from_numpy(emb), exp, ids, rep, prior, H.leave_one_out(3))
    with pytest.raises(ValueError, match="GPU"):
        H.holdout_logits(torch.from_numpy(emb), torch.zeros(3, 5, 16), np.zeros(emb.shape[0], dtype=np.int32))
