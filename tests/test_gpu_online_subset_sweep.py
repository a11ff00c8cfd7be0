"""The grasp-set search on the MI355X (contrastiveprosthetics_amd/online.py sweep_subsets and search_grasp_sets,
csrc/online_subsets.cuh os_rows_kernel and os_sweep_kernel) against its definition `score_subset` (numpy, itself checked by hand
and against a row-by-row loop in tests/test_online_subset_sweep_host.py), and against the shipped gate on the device.  Every
comparison is exact integer equality and nothing is excluded."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("n_cue", "hit", "voted_hit", "classes_scored", "worst_class", "worst_hit", "worst_n")
M = 600
VOTES = (1, 25, 64, 256)


# ---------------------------------------------------------------------------------------------------------------------------
# a cued recording's logits, subsets and the oracle (host only)
# ---------------------------------------------------------------------------------------------------------------------------
def recording(K, m=M, seed=0, rest=True):
    """ids (K,), logits (m, K) f32 uniform in [-1, 1] in steps of 1/8 (ties are common) and expected (m,): cue segments of 10..40
    windows of random classes, with REST and IGNORE stretches of 0..12 windows between them (rest=False: cues only)"""
    from contrastiveprosthetics_amd.online import IGNORE, REST
    rng = np.random.default_rng(1000 * K + seed)
    ids = np.sort(rng.choice(200, K, replace=False)).astype(np.int64)
    lg = (rng.integers(-8, 9, (m, K)) / 8).astype(F)
    exp = np.full(m, IGNORE, dtype=np.int64)
    j = 0
    while j < m:
        n = int(rng.integers(10, 41))
        exp[j:j + n] = ids[int(rng.integers(K))]
        j += n
        if rest:
            r = int(rng.integers(0, 13))
            exp[j:j + r] = REST
            j += r + int(rng.integers(0, 13))                      # (what is not written stays IGNORE)
    return ids, lg, exp


def subsets_of(ids):
    """every subset for K <= 5; else 300 random ones of random size, every singleton and the full set"""
    K = len(ids)
    if K <= 5:
        return [[int(ids[i]) for i in c] for n in range(1, K + 1) for c in itertools.combinations(range(K), n)]
    rng = np.random.default_rng(7 * K)
    out = [[int(c) for c in rng.choice(ids, int(rng.integers(1, K + 1)), replace=False)] for _ in range(300)]
    return out + [[int(c)] for c in ids] + [[int(c) for c in ids]]


def oracle(ids, lg, exp, subsets, vote):
    """score_subset of every subset -> ({key: (G,) int64}, hits (G, K) int64)"""
    from contrastiveprosthetics_amd.online import score_subset
    got = [score_subset(lg, exp, ids, s, vote=vote, per_class=True) for s in subsets]
    return {k: np.array([g[0][k] for g in got], dtype=np.int64) for k in KEYS + ("size",)}, np.stack([g[1] for g in got])


@functools.lru_cache(maxsize=None)
def case(K):
    ids, lg, exp = recording(K)
    for a in (ids, lg, exp):
        a.setflags(write=False)
    return ids, lg, exp, subsets_of(ids)


@functools.lru_cache(maxsize=None)
def answer(K, vote):
    """the oracle's answer for the recording of K classes, computed once and left unchanged"""
    ids, lg, exp, subsets = case(K)
    want, hits = oracle(ids, lg, exp, subsets, vote)
    for a in (hits, *want.values()):
        a.setflags(write=False)
    return want, hits


def sweep(lg_dev, exp, ids, subsets, vote):
    from contrastiveprosthetics_amd.online import sweep_subsets
    scores, hits = sweep_subsets(lg_dev, exp, ids, subsets, vote=vote, per_class=True)
    assert tuple(scores) == KEYS + ("size",) and hits.dtype == torch.int32 and hits.shape == (len(subsets), len(ids))
    return scores, hits.cpu().numpy()


def assert_equal(got, got_hits, want, want_hits, what):
    for k in KEYS + ("size",):
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (what, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    bad = np.argwhere(got_hits != want_hits)
    assert bad.shape[0] == 0, (what, "class hits", bad[:5])


# ---------------------------------------------------------------------------------------------------------------------------
# A. random sets over the range
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vote", VOTES)
@pytest.mark.parametrize("K,ldl", [(1, 1), (2, 2), (5, 5), (41, 41), (64, 64), (5, 64)])
def test_scores_and_class_hits_against_the_definition(K, ldl, vote):
    ids, lg, exp, subsets = case(K)
    want, want_hits = answer(K, vote)
    if K >= 5:                                                         # the data makes every counter work
        assert (want["hit"] != want["voted_hit"]).any() == (vote > 1) and np.unique(want["worst_class"]).size >= 3
        assert (want["classes_scored"] < want["size"]).any() or K == 5
        assert 0 < want["worst_hit"].max() and (want["worst_hit"] < want["worst_n"]).any()
    dev = torch.zeros(M, ldl, device="cuda")
    dev[:, :K] = torch.tensor(lg)
    view = dev[:, :K]                                                  # K < ldl: the rows as a multi-stream push packs them
    assert view.stride(0) == ldl
    got, hits = sweep(view, exp, ids, subsets, vote)
    assert_equal(got, hits, want, want_hits, (K, ldl, vote))
    from contrastiveprosthetics_amd.online import sweep_subsets
    alone = sweep_subsets(view, exp, ids, subsets, vote=vote)          # without the class hits: the same table
    assert all(np.array_equal(alone[k], want[k]) for k in KEYS)


# ---------------------------------------------------------------------------------------------------------------------------
# B. boundaries: the 64-row block, the workgroup of four subsets, rows that are not kept, a ring that never fills
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 128, 257])
def test_block_edges(m):
    ids, lg, exp, subsets = case(5)
    lg, exp = lg[:m], exp[:m]
    dev = torch.tensor(lg).cuda()
    for vote in (1, 3, 64, 256):
        want, want_hits = oracle(ids, lg, exp, subsets, vote)
        got, hits = sweep(dev, exp, ids, subsets, vote)
        assert_equal(got, hits, want, want_hits, (m, vote))


def test_a_subset_does_not_depend_on_its_neighbours():
    ids, lg, exp, subsets = case(41)
    want, want_hits = answer(41, 25)
    t = 5
    assert want["voted_hit"][t] > 0 and 1 < want["size"][t] < 41
    others = subsets[:t] + subsets[t + 1:]
    dev = torch.tensor(lg).cuda()
    places = {"alone": ([subsets[t]], 0)}
    for n in (255, 256, 257):                                          # 64 workgroups less one subset, exactly, and one more
        places[f"first of {n}"] = ([subsets[t]] + others[:n - 1], 0)
        places[f"middle of {n}"] = (others[:n // 2] + [subsets[t]] + others[n // 2:n - 1], n // 2)
        places[f"last of {n}"] = (others[:n - 1] + [subsets[t]], n - 1)
    for name, (subs, at) in places.items():
        got, hits = sweep(dev, exp, ids, subs, 25)
        assert all(got[k][at] == want[k][t] for k in KEYS), name
        assert np.array_equal(hits[at], want_hits[t]), name
        if name == "last of 257":                                      # and the neighbours are themselves
            assert all(np.array_equal(got[k][:t], want[k][:t]) for k in KEYS) and np.array_equal(hits[:t], want_hits[:t])


def test_subsets_with_no_kept_row_and_with_fewer_kept_rows_than_the_vote():
    ids, lg, exp = recording(41, m=300, seed=3, rest=False)            # cues only: a subset keeps the rows of its classes alone
    cued = np.unique(exp)
    never = [int(c) for c in ids if c not in cued]
    assert (exp >= 0).all() and len(never) >= 2 and len(cued) >= 5
    rows_of = {int(c): int((exp == c).sum()) for c in cued}
    few = min(rows_of, key=rows_of.get)
    subsets = [never[:1], never, [few], [few, never[0]], [int(c) for c in cued[:3]], [int(c) for c in ids]]
    for vote in (25, 256):
        assert rows_of[few] < vote
        want, want_hits = oracle(ids, lg, exp, subsets, vote)
        assert want["n_cue"].tolist()[:3] == [0, 0, rows_of[few]] and want["worst_class"].tolist()[:2] == [-1, -1]
        got, hits = sweep(torch.tensor(lg).cuda(), exp, ids, subsets, vote)
        assert_equal(got, hits, want, want_hits, vote)


# ---------------------------------------------------------------------------------------------------------------------------
# C. against the shipped gate with every gate open
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vote", [25, 7])
def test_voted_hits_equal_the_shipped_gate_over_the_kept_rows(vote):
    from contrastiveprosthetics_amd.online import sweep_gate
    ids, lg, exp, subsets = case(41)
    assert np.isfinite(lg).all() and np.abs(lg).max() <= 1.0
    pick = [s for s in subsets[:40] if 1 < len(s) < 41][:20]
    assert len(pick) == 20
    dev = torch.tensor(lg).cuda()
    got, hits = sweep(dev, exp, ids, pick, vote)
    for g, sub in enumerate(pick):
        ids_s = np.array(sorted(sub), dtype=np.int64)
        keep = (exp < 0) | np.isin(exp, ids_s)
        cols = np.searchsorted(ids, ids_s)
        gate, cmds = sweep_gate(dev[torch.from_numpy(keep).cuda()][:, torch.from_numpy(cols).cuda()].contiguous(), exp[keep], ids_s,
                                [dict(vote=vote)], return_commands=True)
        assert gate["hit"][0] == got["voted_hit"][g] and gate["n_cue"][0] == got["n_cue"][g], (g, sub)
        cmd = cmds[0].cpu().numpy()
        per = np.zeros(41, dtype=np.int64)
        per[cols] = [int(((cmd == c) & (exp[keep] == c)).sum()) for c in ids_s]
        assert np.array_equal(per, hits[g]), (g, sub)
    assert got["voted_hit"].max() > 0 and (got["voted_hit"] != got["hit"]).any()


# ---------------------------------------------------------------------------------------------------------------------------
# D. non-finite rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 41])
def test_non_finite_rows_take_a_ring_place_and_never_hit(K):
    ids, lg, exp, subsets = case(K)
    m = 300
    lg, exp, subsets = lg[:m].copy(), exp[:m], subsets[:80]
    rng = np.random.default_rng(9)
    rows = rng.choice(m, 40, replace=False)                            # (with all subsets of 5, or 80 random ones of 41, every bad
    lg[rows[:20], rng.integers(0, K, 20)] = np.nan                     # column is inside some subsets and outside others)
    lg[rows[20:32], rng.integers(0, K, 12)] = np.inf
    lg[rows[32:]] = np.inf                                             # whole rows
    plain, _ = oracle(ids, case(K)[1][:m], exp, subsets, 25)
    for vote in (1, 25):
        want, want_hits = oracle(ids, lg, exp, subsets, vote)
        got, hits = sweep(torch.tensor(lg).cuda(), exp, ids, subsets, vote)
        assert_equal(got, hits, want, want_hits, ("non-finite", K, vote))
    assert (want["hit"] < plain["hit"]).any() and (want["voted_hit"] != plain["voted_hit"]).any()     # the rows matter


# ---------------------------------------------------------------------------------------------------------------------------
# E. device values the wrapper would refuse, written straight to the arrays
# ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_masks_score_minus_one_and_invalid_cues_are_unscored():
    """a validity check of what the kernel does with values it must not index with; checked by value"""
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import IGNORE
    ids, lg, exp, subsets = case(5)
    lib = _lib.load()
    K, vote = 5, 25
    masks = np.array([0b00111, 0, 0b10001, 1 << 5, 0b11111, 1 << 63, 0b01000 | 1 << 40], dtype=np.uint64)   # two workgroups
    valid = [0, 2, 4]
    slot = {int(c): k for k, c in enumerate(ids)}
    slots = np.array([slot.get(int(e), int(e)) for e in exp], dtype=np.int32)
    cue_rows = np.nonzero(slots >= 0)[0]
    stray = cue_rows[::7]
    slots[stray] = np.resize([5, 6, 64, 2 ** 30, 2 ** 31 - 1], stray.shape[0])    # slots the recording does not have
    as_ignored = exp.copy()
    as_ignored[stray] = IGNORE
    want, want_hits = oracle(ids, lg, as_ignored, [[int(ids[k]) for k in range(K) if int(masks[g]) >> k & 1] for g in valid], vote)
    dev, exp_d = torch.tensor(lg).cuda(), torch.from_numpy(slots).cuda()
    masks_d = torch.from_numpy(masks.view(np.int64)).cuda()
    scratch = torch.empty(lib.cp_online_subset_sweep_scratch_bytes(M), dtype=torch.uint8, device="cuda")
    scores = torch.full((len(masks), 7), -99, dtype=torch.int64, device="cuda")
    hits = torch.full((len(masks), 64), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.cp_online_subset_sweep(dev.data_ptr(), K, M, K, exp_d.data_ptr(), masks_d.data_ptr(), len(masks), vote,
                                          scratch.data_ptr(), scratch.numel(), scores.data_ptr(), hits.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "cp_online_subset_sweep")
    scores, hits = scores.cpu().numpy(), hits.cpu().numpy()
    for g in range(len(masks)):
        if g not in valid:
            assert (scores[g] == -1).all() and (hits[g] == -7).all(), g
        else:                                                          # the worst class is a slot here, a class id in the oracle
            i = valid.index(g)
            w = [int(want[k][i]) for k in KEYS]
            w[4] = slot[w[4]] if w[4] >= 0 else -1
            assert scores[g].tolist() == w, g
            assert np.array_equal(hits[g, :K], want_hits[i]) and (hits[g, K:] == 0).all(), g


# ---------------------------------------------------------------------------------------------------------------------------
# F. the search end to end
# ---------------------------------------------------------------------------------------------------------------------------
def confusable_recording(m=800):
    """K = 8; the cued class is raised by 0.5 over noise of width 0.4, and classes 11 and 30 (slots 2 and 5) share the raise
    whichever of the two is cued: that pair is confusable by construction"""
    from contrastiveprosthetics_amd.online import IGNORE, REST
    rng = np.random.default_rng(5)
    ids = np.array([3, 7, 11, 12, 20, 30, 31, 40], dtype=np.int64)
    lg = (rng.integers(-16, 17, (m, 8)) / 80).astype(F)
    exp = np.full(m, IGNORE, dtype=np.int64)
    for i, j in enumerate(range(0, m, 25)):
        c = i % 8
        lg[j:j + 20, c] += F(0.5)
        if c in (2, 5):
            lg[j:j + 20, 7 - c] += F(0.5)
        exp[j:j + 20] = ids[c]
        exp[j + 21:j + 25] = REST
    return ids, lg, exp


def test_search_grasp_sets_avoids_a_confusable_pair_and_equals_the_host_ranking():
    from contrastiveprosthetics_amd.online import rank_subsets, score_subset, search_grasp_sets
    ids, lg, exp = confusable_recording()
    dev = torch.tensor(lg).cuda()
    found = search_grasp_sets(dev, exp, ids, min_size=2, max_size=4, vote=9, keep=5)
    assert [(r["size"], r["exhaustive"], r["n_candidates"]) for r in found] == [(2, True, 28), (3, True, 56), (4, True, 70)]
    for r in found:
        best_ids, best = r["best"][0]
        assert not {11, 30} <= set(best_ids) and best["classes_scored"] == r["size"], r["best"][0]
        combos = [tuple(int(ids[i]) for i in c) for c in itertools.combinations(range(8), r["size"])]
        table = [score_subset(lg, exp, ids, c, vote=9) for c in combos]
        order = rank_subsets({k: np.array([t[k] for t in table]) for k in KEYS + ("size",)})
        assert r["best"] == [(combos[g], table[g]) for g in order[:5]]
        both = [t for c, t in zip(combos, table) if {11, 30} <= set(c)]
        assert max(t["worst_hit"] / t["worst_n"] for t in both) < best["worst_hit"] / best["worst_n"]
    beamed = search_grasp_sets(dev, exp, ids, min_size=2, max_size=5, vote=9, require=[30, 7], exhaustive=1, beam=3, keep=4)
    assert [(r["size"], r["exhaustive"]) for r in beamed] == [(2, True), (3, False), (4, False), (5, False)]
    assert [r["n_candidates"] for r in beamed][:2] == [1, 6]
    for r in beamed:
        assert r["best"] and all({30, 7} <= set(s) and len(s) == r["size"] for s, _ in r["best"])
        for s, sc in r["best"]:
            assert sc == score_subset(lg, exp, ids, s, vote=9)
