"""Posture prototypes without a GPU (contrastiveprosthetics_amd/prototypes.py, include/cpnative.h cp_online_proto_fit and
cp_online_group_*): the properties of the numpy definitions `fit_reference` and `group_reference`, the table an install
builds, the point of the synthetic posture recording, and the binding and host checks of the C entries."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import prototypes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG = 10001
F = np.float32
ENTRIES = ["cp_online_proto_fit", "cp_online_group_set_groups", "cp_online_group_reset", "cp_online_group_push"]
R, I = P.REST, P.IGNORE


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def person(seed=0, m=1800, k=4, postures=2):
    """the posture recording, its repetitions and the training mask: every repetition but the last of each posture"""
    emb, exp, pos = P.posture_recording(m, k, postures, seed=seed, segment=30, rest=8)
    rep, n_rep = H.repetitions(exp)
    return emb, exp, pos, np.arange(k), rep < n_rep - postures


# ---------------------------------------------------------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_row_per_class_is_the_zero_prior_enrolment_row_for_any_iters():
    emb, exp, _, ids, use = person()
    rep, n_rep = H.repetitions(exp)
    mask = sum(1 << r for r in range(n_rep - 2))
    prior = np.eye(4, 16, dtype=F)                             # (the sums do not depend on it)
    sums = H.holdout_reference(emb, exp, ids, rep, prior, [dict(train=mask, eval=0, mix=1.0, min_windows=10)])["sums"][0]
    want = np.zeros((4, 16), dtype=F)
    for c in range(4):
        s2 = np.float64(0.0)
        for d in range(16):
            s2 = s2 + sums[c, d] * sums[c, d]
        want[c] = (sums[c] / np.sqrt(s2)).astype(F)            # ole_table_kernel with a zero prior at mix = 1
    # a window trains there iff its repetition is in the mask; rest windows carry a repetition too but no class
    for iters in (0, 1, 7):
        fit = P.fit_reference(emb, exp, ids, 1, iters=iters, min_windows=10, use=use)
        assert same_bits(fit["rows"][:, 0], want), iters
        assert fit["valid"][:, 0].all() and not fit["valid"][:, 1:].any() and not fit["rows"][:, 1:].any()
        assert (fit["moved"][:, 1:] == 0).all() and (fit["moved"][:, :1] == fit["counts"][:, :1]).all()
        assert (fit["assign"][use & (exp >= 0)] == 0).all() and (fit["assign"][~(use & (exp >= 0))] == -1).all()


def test_moved_reaches_zero_and_the_rows_then_stop_changing():
    emb, exp, _, ids, use = person(seed=3)
    full = P.fit_reference(emb, exp, ids, 3, iters=64, min_windows=1, use=use)
    assert (full["moved"][:, 0] == full["counts"].sum(axis=1)).all()
    assert (full["moved"][:, -1] == 0).all(), "64 rounds do not settle this recording: pick another"
    for c in range(4):
        t0 = int(np.nonzero(full["moved"][c] == 0)[0][0])      # the first round that moves nothing
        assert (full["moved"][c, t0:] == 0).all()
        short = P.fit_reference(emb, exp, ids, 3, iters=t0 + 1, min_windows=1, use=use)
        assert same_bits(short["rows"][c], full["rows"][c]) and same_bits(short["counts"][c], full["counts"][c])
    assert same_bits(np.nonzero(full["assign"] >= 0)[0], np.nonzero(use & (exp >= 0))[0])


def test_farthest_first_copies_windows_and_ties_go_to_the_earliest():
    rng = np.random.default_rng(5)
    base = rng.standard_normal((3, 16)).astype(F)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    emb = np.concatenate([base, base, base[::-1]]).astype(F)   # every window three times: ties everywhere
    exp = np.zeros(9, dtype=np.int64)
    fit = P.fit_reference(emb, exp, [0], 3, iters=0, min_windows=1)
    s = emb.astype(np.float64).sum(axis=0)
    near = emb @ (s / np.linalg.norm(s)).astype(F)
    assert same_bits(fit["rows"][0, 1], emb[int(np.argmin(near))])          # a window, bit for bit
    assert any(same_bits(fit["rows"][0, 2], e) for e in emb[:3])
    # duplicates of a centre tie in the assignment and go to the first of the tied centres
    two = P.fit_reference(np.stack([base[0], base[0]]), np.zeros(2, dtype=np.int64), [0], 4, iters=2, min_windows=1)
    assert two["counts"][0].tolist() == [2, 0, 0, 0] and two["valid"][0].tolist() == [True, False, False, False]
    assert two["assign"].tolist() == [0, 0]


def test_windows_that_do_not_train_and_classes_that_are_not_fitted():
    emb, exp, _, ids, use = person(seed=1)
    exp = exp.copy()
    exp[5:9] = I
    cue0 = np.nonzero((exp == 0) & use)[0]
    emb[cue0[3], 4] = np.nan
    emb[cue0[7], 0] = np.inf
    emb[cue0[9]] = 0.0                                         # an all-zero window is finite: it trains
    few = np.nonzero((exp == 2) & use)[0][6:]                  # class 2 keeps six windows: below min_windows
    use = use.copy()
    use[few] = False
    fit = P.fit_reference(emb, exp, np.array([0, 1, 2, 3, 9]), [2, 1, 2, 4, 3], iters=5, min_windows=10, use=use)
    assert fit["assign"][cue0[3]] == -1 and fit["assign"][cue0[7]] == -1 and fit["assign"][cue0[9]] >= 0
    assert fit["counts"][0].sum() == cue0.size - 2 and np.isfinite(fit["rows"]).all()
    assert not fit["valid"][2].any() and not fit["rows"][2].any() and (fit["assign"][exp == 2] == -1).all()
    assert not fit["valid"][4].any() and fit["counts"][4].sum() == 0          # class 9 is absent from the recording
    assert (fit["assign"][exp < 0] == -1).all() and (fit["assign"][~use] == -1).all()
    assert fit["valid"][3].sum() < 4 or fit["counts"][3].min() >= 10          # a centre below min_windows is dropped
    assert (fit["valid"] == ((fit["counts"] >= 10) & (np.arange(4)[None] < np.array([2, 1, 2, 4, 3])[:, None]))).all()
    # one class alone gives what the full fit gives for it
    for c, cid, r in ((0, 0, 2), (3, 3, 4)):
        alone = P.fit_reference(emb, np.where(exp == cid, exp, R), [cid], r, iters=5, min_windows=10, use=use)
        assert same_bits(alone["rows"][0], fit["rows"][c]) and same_bits(alone["counts"][0], fit["counts"][c])
        assert same_bits(alone["moved"][0], fit["moved"][c]) and same_bits(alone["assign"][exp == cid], fit["assign"][exp == cid])


def test_a_dropped_centre_is_never_installed():
    emb, exp, _, ids, use = person(seed=0)
    fit = P.fit_reference(emb, exp, ids, 2, iters=10, min_windows=10, use=use)
    assert fit["valid"][0, :2].all() and not fit["valid"][:, :2].all(), "the recording should drop a centre of a one-posture class"
    table, rid = P.prototype_table(ids, fit["rows"], fit["valid"])
    want = [P.row_id(c, q) for c in range(4) for q in range(4) if fit["valid"][c, q]]
    assert rid.tolist() == want == sorted(want) and table.shape == (len(want), 16)
    for j, r in enumerate(rid.tolist()):
        assert same_bits(table[j], fit["rows"][P.class_of_row(r), r % 4])
    assert [P.class_of_row(r) for r in rid.tolist()] == sorted(P.class_of_row(r) for r in rid.tolist())
    # a class with no valid centre takes the current row under the id 4 c, and needs one
    valid = fit["valid"].copy()
    valid[1] = False
    cur = np.arange(64, dtype=F).reshape(4, 16)
    table, rid = P.prototype_table(ids, fit["rows"], valid, cur)
    at = rid.tolist().index(4)
    assert same_bits(table[at], cur[1]) and 5 not in rid.tolist()
    assert same_bits(P.prototype_table(ids, fit["rows"], valid, {1: cur[1]})[0], table)
    with pytest.raises(ValueError, match="not fitted"):
        P.prototype_table(ids, fit["rows"], valid)
    with pytest.raises(ValueError, match="not fitted"):
        P.prototype_table(ids, fit["rows"], valid, {0: cur[0]})
    pr = P.Prototypes.of(fit)
    assert pr.fitted.all() and same_bits(pr.table()[1], P.prototype_table(ids, fit["rows"], fit["valid"])[1])


def test_the_fit_refuses_what_it_cannot_take():
    emb, exp, _, ids, _ = person(m=200)
    for bad in (0, 5, -1, True, 2.0, [1, 2, 3], [1, 1, 1, 5], [[1, 1, 1, 1]]):
        with pytest.raises(ValueError, match="rows_per_class"):
            P.fit_reference(emb, exp, ids, bad)
    with pytest.raises(ValueError, match="at most 64"):
        P.fit_reference(emb, np.full(200, R), np.arange(17), 4)
    P.fit_reference(emb, np.full(200, R), np.arange(16), 4, iters=0)           # 64 rows are allowed
    for bad in (-1, 65, 1.5, True):
        with pytest.raises(ValueError, match="iters"):
            P.fit_reference(emb, exp, ids, 2, iters=bad)
    for bad in (0, -3, 2 ** 31):
        with pytest.raises(ValueError, match="min_windows"):
            P.fit_reference(emb, exp, ids, 2, min_windows=bad)
    for bad in ([1, 0, 2, 3], [0, 1, 1, 2], [-1, 0, 1, 2]):
        with pytest.raises(ValueError, match="ascending"):
            P.fit_reference(emb, exp, bad, 2)
    with pytest.raises(ValueError, match="use"):
        P.fit_reference(emb, exp, ids, 2, use=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="expected"):
        P.fit_reference(emb, np.where(exp == 0, 7, exp), ids, 2)
    with pytest.raises(ValueError, match="embeddings"):
        P.fit_reference(emb[:, :8], exp, ids, 2)
    with pytest.raises(ValueError, match="row id"):
        P.prototype_table([2 ** 29], np.zeros((1, 4, 16), F), np.ones((1, 4), bool))
    assert P.row_id(7, 3) == 31 and P.class_of_row(31) == 7
    with pytest.raises(ValueError):
        P.row_id(7, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------------------------------------------------------
def test_group_reference_with_singleton_groups_is_the_decoders_tail():
    rng = np.random.default_rng(2)
    l = rng.standard_normal((300, 7)).astype(F)
    l[10, 2] = l[10, 5] = l[10].max() + 1                      # a tie: the smallest id
    rid = np.array([3, 4, 9, 10, 11, 40, 41])
    g = P.group_reference(l, rid, None, vote=5)
    assert same_bits(g["logits"], l) and g["ids"].tolist() == rid.tolist()
    assert g["pred"].tolist() == rid[l.argmax(axis=1)].tolist() == g["row"].tolist() and g["pred"][10] == 9
    ring, voted = [], []
    for p in l.argmax(axis=1).tolist():
        ring = (ring + [p])[-5:]
        voted.append(rid[np.bincount(ring, minlength=7).argmax()])
    assert g["voted"].tolist() == voted


def test_group_reference_takes_the_maximum_of_a_groups_rows():
    l = np.array([[0.1, 0.9, 0.3, 0.2],                        # class 2's second row wins
                  [0.5, 0.5, 0.5, 0.5],                        # all equal: the smallest group, its first row
                  [0.1, np.nan, 0.3, 0.2],                     # a NaN: nothing is predicted, class 2's logit is a NaN
                  [0.1, 0.2, np.inf, 0.2],                     # an Inf: nothing is predicted, the logit is written
                  [-0.0, 0.0, -1.0, -2.0],
                  [0.0, 0.1, 0.2, 0.7]], dtype=F)
    rid = np.array([8, 9, 20, 23])                             # class 2: rows 8, 9; class 5: rows 20, 23
    g = P.group_reference(l, rid, vote=3)
    assert g["ids"].tolist() == [2, 5]
    assert g["pred"].tolist() == [2, 2, -1, -1, 2, 5] and g["row"].tolist() == [9, 8, -1, -1, 8, 23]
    assert g["voted"].tolist() == [2, 2, 2, 2, 2, 2]           # ring of 3: (2), (2, 2), (2, 2, -), (2, -, -), (-, -, 2), (-, 2, 5)
    assert np.isnan(g["logits"][2, 0]) and g["logits"][2, 1] == F(0.3) and g["logits"][3].tolist() == [F(0.2), np.inf]
    assert same_bits(g["logits"][[0, 1, 5]], np.array([[0.9, 0.3], [0.5, 0.5], [0.1, 0.7]], dtype=F))
    assert same_bits(g["logits"][4, :1], np.array([-0.0], dtype=F))             # the first of -0 and +0
    none = P.group_reference(np.full((4, 4), np.nan, dtype=F), rid, vote=3)
    assert none["pred"].tolist() == none["voted"].tolist() == none["row"].tolist() == [-1] * 4
    # a dict names some rows, the others are their own class; R class ids name all
    d = P.group_reference(l, rid, {8: 1, 9: 1}, vote=3)
    assert d["ids"].tolist() == [1, 20, 23] and d["pred"][0] == 1
    a = P.group_reference(l, rid, [7, 7, 7, 3], vote=3)
    assert a["ids"].tolist() == [3, 7] and a["pred"].tolist()[:2] == [7, 3]
    for bad in (0, 257):
        with pytest.raises(ValueError, match="vote"):
            P.group_reference(l, rid, vote=bad)
    with pytest.raises(ValueError, match="logits"):
        P.group_reference(l[:, :3], rid)
    with pytest.raises(ValueError, match="class ids"):
        P.group_reference(l, rid, lambda r: -1)


def test_two_rows_decode_the_postures_that_one_row_cannot():
    """train on every repetition but the last of each posture, decode the held-out ones through the definitions"""
    emb, exp, pos, ids, use = person(seed=0)
    held = ~use
    cue = exp[held] >= 0
    hits = {}
    for rows in (1, 2):
        fit = P.fit_reference(emb, exp, ids, rows, iters=10, min_windows=10, use=use)
        table, rid = P.prototype_table(ids, fit["rows"], fit["valid"])
        g = P.group_reference(P.row_logits_reference(emb[held], table), rid, vote=9)
        assert g["ids"].tolist() == ids.tolist()
        hits[rows] = int((g["voted"][cue] == exp[held][cue]).sum())
        if rows == 2:                                          # class 0's two rows are its two arm positions
            a = fit["assign"][use & (exp == 0)]
            p = pos[use & (exp == 0)]
            assert (a == a[0]).sum() == (p == p[0]).sum() and ((a == a[0]) == (p == p[0])).all()
    assert hits[2] > hits[1]


def test_the_stage_derives_its_groups_from_the_decoders_ids_without_a_device():
    class Fake:
        class_ids, n_seen, vote, ws, device = None, 0, 25, None, None

        def push(self, *a, **k):
            raise AssertionError
    dec = Fake()
    stage = P.PostureRows(dec)
    assert stage.class_ids is None and stage.vote == 25 and stage.n_seen == 0 and not stage.multi
    dec.class_ids = np.array([0, 1, 8, 9, 10, 44], dtype=np.int32)
    first = stage.class_ids
    assert first.tolist() == [0, 2, 11] and stage.class_ids is first and stage.row_ids().tolist() == [0, 1, 8, 9, 10, 44]
    dec.class_ids = dec.class_ids.copy()                       # a new object: derived again, a new object here too
    assert stage.class_ids is not first and stage.class_ids.tolist() == [0, 2, 11]
    stage.set_class_of_row(None)
    assert stage.class_ids.tolist() == [0, 1, 8, 9, 10, 44]
    multi = Fake()
    multi.class_ids, multi.n_seen = [None, np.array([4, 5, 12])], np.zeros(2, dtype=np.int64)
    st = P.PostureRows(multi, [None, P.class_of_row])
    assert st.multi and st.class_ids[0] is None and st.class_ids[1].tolist() == [1, 3]
    with pytest.raises(ValueError, match="class_of_row"):
        P.PostureRows(multi, [None])
    with pytest.raises(TypeError):
        P.PostureRows(object())
    dec.n_seen = 40
    with pytest.raises(Exception, match="behind the posture stage"):
        stage.push(None)


def test_posture_recording_is_repeatable_and_straddles():
    a, b = P.posture_recording(500, 3, 3, seed=4), P.posture_recording(500, 3, 3, seed=4)
    assert all(same_bits(x, y) for x, y in zip(a, b)) and a[0].dtype == F and a[0].shape == (500, 16)
    emb, exp, pos = a
    assert np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-6) and set(exp.tolist()) == {R, 0, 1, 2}
    assert set(pos[exp >= 0].tolist()) == {0, 1, 2} and (pos[exp == R] == -1).all()
    mean = lambda sel: emb[sel].astype(np.float64).mean(axis=0)
    unit = lambda v: v / np.linalg.norm(v)
    u = unit(mean(exp == 1))
    assert unit(mean(exp == 0)) @ u > 0.97                     # the mean of class 0 falls on class 1
    assert unit(mean((exp == 0) & (pos == 0))) @ u < 0.8 and unit(mean((exp == 0) & (pos == 2))) @ u < 0.8
    with pytest.raises(ValueError):
        P.posture_recording(100, 1)


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
    assert hasattr(raw, "cp_online_group_workspace_bytes") and "cp_online_group_workspace_bytes" in _lib.SYMBOLS
    for name in ("CP_ONLINE_PROTO_MAX_ROWS", "CP_ONLINE_PROTO_MAX_ITERS"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(_lib, name), name
    assert P.MAX_ROWS == 4 and P.MAX_ITERS == 64
    one = lib.cp_online_group_workspace_bytes(1)
    assert one == (P._OPG_WORDS * 4 + 255) // 256 * 256 == lib.cp_online_group_workspace_bytes(0)
    assert lib.cp_online_group_workspace_bytes(256) == 256 * P._OPG_WORDS * 4


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory for every pointer: each refusal returns before a launch, which on a machine without a GPU would fail otherwise"""
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    M, K = 8, 3
    rpc = (ctypes.c_int32 * 64)(*([2] * 64))

    def err(rc, entry, what):
        assert rc == ERR_ARG, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    def fit(emb=p, m=M, k=K, slot=p, use=None, rows_per_class=rpc, iters=3, minw=5, rows=p, counts=p, valid=p, moved=p, assign=p):
        return lib.cp_online_proto_fit(emb, m, k, slot, use, rows_per_class, iters, minw, rows, counts, valid, moved, assign, None)

    name = "cp_online_proto_fit"
    for m in (0, -1, 2 ** 31):
        err(fit(m=m), name, "n_rows")
    for k in (0, 65, -1):
        err(fit(k=k), name, "n_classes")
    for it in (-1, 65):
        err(fit(iters=it), name, "iters")
    for mw in (0, -1):
        err(fit(minw=mw), name, "min_windows")
    for arg in ("emb", "slot", "rows_per_class", "rows", "counts", "valid", "moved", "assign"):
        err(fit(**{arg: None}), name, "required")
    for arg in ("slot", "rows", "counts", "moved", "assign"):
        err(fit(**{arg: p + 2}), name, "misaligned")
    err(fit(counts=p + 4), name, "misaligned")
    err(fit(emb=p + 8), name, "16-byte")
    for bad in (0, 5, -1):
        err(fit(rows_per_class=(ctypes.c_int32 * 3)(2, bad, 1)), name, "rows_per_class outside")
    err(fit(k=33), name, "more than 64 rows")

    S = 3
    need = lib.cp_online_group_workspace_bytes(S)
    ids = (ctypes.c_int32 * 3)(4, 5, 8)
    cls = (ctypes.c_int32 * 3)(1, 1, 2)
    sg, rs, pu = "cp_online_group_set_groups", "cp_online_group_reset", "cp_online_group_push"

    def entries(vote=25, n_streams=S, w=p, nbytes=need):
        return ((sg, lambda: lib.cp_online_group_set_groups(vote, n_streams, w, nbytes, 0, ids, cls, 3, None)),
                (rs, lambda: lib.cp_online_group_reset(vote, n_streams, w, nbytes, -1, None)),
                (pu, lambda: lib.cp_online_group_push(vote, n_streams, w, nbytes, p, 3, p, p, 1, p, p, p, None, 0, None)))

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
    for entry, call in entries(nbytes=need - 256):
        err(call(), entry, "too small")
    for n in (0, 65):
        err(lib.cp_online_group_set_groups(25, S, p, need, 0, ids, cls, n, None), sg, "rows")
    err(lib.cp_online_group_set_groups(25, S, p, need, 0, None, cls, 3, None), sg, "rows")
    err(lib.cp_online_group_set_groups(25, S, p, need, 0, ids, None, 3, None), sg, "rows")
    err(lib.cp_online_group_set_groups(25, S, p, need, S, ids, cls, 3, None), sg, "stream index")
    err(lib.cp_online_group_set_groups(25, S, p, need, -1, ids, cls, 3, None), sg, "stream index")
    for bad in ((5, 4, 8), (4, 4, 8), (-1, 4, 8), (4, 5, 2 ** 31 - 1)):
        err(lib.cp_online_group_set_groups(25, S, p, need, 0, (ctypes.c_int32 * 3)(*bad), cls, 3, None), sg, "ascending")
    for bad in ((-1, 1, 2), (1, 1, 2 ** 31 - 1)):
        err(lib.cp_online_group_set_groups(25, S, p, need, 0, ids, (ctypes.c_int32 * 3)(*bad), 3, None), sg, "class ids")
    err(lib.cp_online_group_reset(25, S, p, need, S, None), rs, "stream index")
    err(lib.cp_online_group_reset(25, S, p, need, -2, None), rs, "stream index")
    push = lambda lg=p, ldl=3, row0=p, m=p, total=1, pred=p, voted=p, row=p, cl=None, ldc=0: \
        lib.cp_online_group_push(25, S, p, need, lg, ldl, row0, m, total, pred, voted, row, cl, ldc, None)
    for total in (-1, 65537):
        err(push(total=total), pu, "total_rows")
    err(push(ldl=0), pu, "ldl")
    err(push(cl=p, ldc=0), pu, "ldc")
    for arg in ("lg", "row0", "m", "pred", "voted", "row"):
        err(push(**{arg: None}), pu, "required")
        err(push(**{arg: p + 2}), pu, "misaligned")
    err(push(cl=p + 2, ldc=4), pu, "misaligned")
    assert lib.cp_online_group_push(25, S, p, need, None, 3, None, None, 0, None, None, None, None, 0, None) == 0     # nothing to do


def test_wrappers_check_before_they_touch_a_device_and_are_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    assert pkg.fit_prototypes is P.fit_prototypes and pkg.fit_reference is P.fit_reference and pkg.PostureRows is P.PostureRows
    assert pkg.group_reference is P.group_reference and pkg.Prototypes is P.Prototypes and pkg.posture_recording is P.posture_recording
    emb, exp, _, ids, _ = person(m=200)
    for kw, what in ((dict(rows_per_class=5), "rows_per_class"), (dict(iters=65), "iters"), (dict(min_windows=0), "min_windows"),
                     (dict(ids=[1, 0, 2, 3]), "ascending")):
        args = dict(embeddings=emb, expected=exp, ids=ids)
        args.update(kw)
        with pytest.raises(ValueError, match=what):            # (before the embeddings are looked at)
            P.fit_prototypes(**args)
    with pytest.raises(ValueError, match="embeddings"):
        P.fit_prototypes(emb, exp, ids)                        # numpy, not a GPU tensor


def test_install_groups_only_its_own_stream_and_finds_current_rows_through_the_stage():
    """`Prototypes.install` on a stand-in multi-stream decoder that keeps what `set_classes` is given"""
    import torch

    class Multi:
        vote, ws, device = 9, None, None

        def __init__(self, n):
            self.class_ids, self.tables, self.n_seen = [None] * n, [None] * n, np.zeros(n, dtype=np.int64)

        def set_classes(self, stream, table=None, ids=None):
            order = np.argsort(np.asarray(ids))
            self.tables[stream] = torch.as_tensor(np.asarray(table, dtype=F))[order]
            self.class_ids[stream] = torch.as_tensor(np.asarray(ids)[order], dtype=torch.int32)

        def class_table(self, stream):
            return self.tables[stream].clone(), self.class_ids[stream].clone()

        def push(self, *a, **k):
            raise AssertionError

    emb, exp, _, ids, use = person(seed=0)
    fit = P.Prototypes.of(P.fit_reference(emb, exp, ids, 2, iters=10, min_windows=10, use=use))
    dec = Multi(3)
    plain = np.arange(41 * 16, dtype=F).reshape(41, 16) + 1
    dec.set_classes(0, table=plain, ids=np.arange(41))
    stage = fit.install(dec, 1)
    assert stage.class_ids[0].tolist() == list(range(41))      # the plain neighbour keeps one class per row
    assert stage.class_ids[1].tolist() == [0, 1, 2, 3] and stage.class_ids[2] is None
    assert dec.class_ids[1].tolist() == fit.table()[1].tolist() and same_bits(dec.tables[1].numpy(), fit.table()[0])
    # a fit with classes that were not fitted takes the decoder's rows of those classes, also once its ids are row ids
    part = P.Prototypes.of(P.fit_reference(emb, np.where(exp == 2, R, exp), np.array([0, 1, 2, 3, 6]), 2, iters=3, min_windows=10, use=use))
    assert part.fitted.tolist() == [True, True, False, True, False]
    with pytest.raises(ValueError, match="not fitted"):
        part.install(dec, 2, stage=stage)                      # stream 2 has no table to fall back on
    assert dec.class_ids[2] is None
    dec.set_classes(2, table=plain[:7], ids=np.arange(7))
    assert part.install(dec, 2, stage=stage) is stage
    first, rid = dec.tables[2].numpy().copy(), dec.class_ids[2].tolist()
    assert 8 in rid and 24 in rid and 9 not in rid and same_bits(first[rid.index(8)], plain[2]) and same_bits(first[rid.index(24)], plain[6])
    assert stage.class_ids[2].tolist() == [0, 1, 2, 3, 6] and stage.class_ids[0].tolist() == list(range(41))
    part.install(dec, 2, stage=stage)                          # the ids are row ids now: the stage says which class a row is
    assert same_bits(dec.tables[2].numpy(), first) and dec.class_ids[2].tolist() == rid
    with pytest.raises(ValueError, match="not fitted"):
        part.install(dec, 2)                                   # without the stage row id 24 is not class 6
    assert same_bits(dec.tables[2].numpy(), first)
    with pytest.raises(ValueError, match="stream"):
        fit.install(dec)
    with pytest.raises(IndexError):
        fit.install(dec, 3)
    with pytest.raises(ValueError, match="stage="):
        fit.install(Multi(3), 0, stage=stage)
