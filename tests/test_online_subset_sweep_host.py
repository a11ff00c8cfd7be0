"""CPU checks of the grasp-set search (contrastiveprosthetics_amd/online.py score_subset, sweep_subsets, rank_subsets,
search_grasp_sets; csrc/online_subsets.cuh): the definition on cases worked out by hand and against a row-by-row loop, the
ranking on every key and on ties, the candidate generation through a scoring callable, the wrapper's refusals through a stubbed
device call, and the two C entries' declarations, sizes and refusals before any device call."""
import ctypes
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ENTRIES = ["cp_online_subset_sweep_scratch_bytes", "cp_online_subset_sweep"]
ERR_ARG = 10001
KEYS = ("n_cue", "hit", "voted_hit", "classes_scored", "worst_class", "worst_hit", "worst_n")
IDS = [2, 5, 7, 9]                                                       # slots 0..3
REST, IGNORE = -1, -2
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------------
# score_subset on cases worked out by hand
# ---------------------------------------------------------------------------------------------------------------------------
def _score(rows, expected, subset, vote, **kw):
    from contrastiveprosthetics_amd.online import SUBSET_SCORE_KEYS, score_subset
    assert SUBSET_SCORE_KEYS == KEYS
    out = score_subset(np.array(rows, dtype=np.float32).reshape(len(expected), len(IDS)), np.array(expected, dtype=np.int64), IDS,
                       subset, vote=vote, **kw)
    sc = out[0] if kw.get("per_class") else out
    assert tuple(sc) == KEYS + ("size",) and all(type(v) is int for v in sc.values()) and sc["size"] == len(set(subset))
    return out


def _want(n_cue, hit, voted_hit, classes_scored, worst_class, worst_hit, worst_n, size):
    return dict(n_cue=n_cue, hit=hit, voted_hit=voted_hit, classes_scored=classes_scored, worst_class=worst_class,
                worst_hit=worst_hit, worst_n=worst_n, size=size)


def test_a_tie_between_two_slots_of_the_subset_goes_to_the_lower_slot():
    row = [0.5, 0.5, 0.0, 0.0]
    assert _score([row], [5], [2, 5], 1) == _want(1, 0, 0, 1, 5, 0, 1, 2)         # predicted 2, cued 5
    assert _score([row], [2], [5, 2], 1) == _want(1, 1, 1, 1, 2, 1, 1, 2)
    assert _score([[0.0, -0.0, 0.0, 0.0]], [5], [5, 7, 9], 1) == _want(1, 1, 1, 1, 5, 1, 1, 3)   # -0.0 == 0.0: still a tie


def test_a_maximum_outside_the_subset_is_ignored():
    row = [0.1, 0.3, 0.9, 0.2]                                           # class 7 has the maximum
    assert _score([row], [5], [2, 5], 1) == _want(1, 1, 1, 1, 5, 1, 1, 2)
    assert _score([row], [5], [2, 5, 7], 1) == _want(1, 0, 0, 1, 5, 0, 1, 3)


FOR_2, FOR_5 = [0.9, 0.1, 0.0, 0.0], [0.1, 0.9, 0.0, 0.0]


def test_a_dropped_row_does_not_enter_the_ring_and_a_rest_row_does():
    rows = [FOR_2, FOR_5, FOR_5, FOR_5]
    # rows 1 and 2 are cued for class 7, which is not kept: the ring at row 3 holds [2, 5], a tie that goes to class 2
    assert _score(rows, [2, 7, 7, 2], [2, 5], 3) == _want(2, 1, 2, 1, 2, 2, 2, 2)
    # the same rows at rest stay in the stream: the ring at row 3 holds [5, 5, 5]
    assert _score(rows, [2, REST, REST, 2], [2, 5], 3) == _want(2, 1, 1, 1, 2, 1, 2, 2)
    assert _score(rows, [2, IGNORE, REST, 2], [2, 5], 3) == _want(2, 1, 1, 1, 2, 1, 2, 2)
    # with class 7 kept they are cue rows of their own: row 3 is a miss again, rows 1 and 2 predict 5 and vote 2 then 5
    assert _score(rows, [2, 7, 7, 2], [2, 5, 7], 3) == _want(4, 1, 1, 2, 7, 0, 2, 3)


def test_a_vote_tie_goes_to_the_smaller_slot():
    for_7 = [0.0, 0.1, 0.9, 0.0]
    # ring of 2: [7] -> 7; [7, 5] -> a tie, class 5; [5, 7] -> class 5 again
    assert _score([for_7, FOR_5, for_7], [7, 7, 7], [5, 7], 2) == _want(3, 2, 1, 1, 7, 1, 3, 2)


def test_a_nan_row_takes_a_ring_place_and_is_never_a_hit():
    bad_outside = [0.9, 0.1, 0.0, NAN]                                   # the NaN is in a column outside the subset
    # ring of 2: [2] -> 2; [2, none] -> 2 (the voted hit of a row that is no raw hit); [none, none] -> none
    assert _score([FOR_2, bad_outside, bad_outside], [2, 2, 2], [2, 5], 2) == _want(3, 1, 2, 1, 2, 2, 3, 2)
    bad_inside = [float("inf"), 0.1, 0.0, 0.0]
    assert _score([FOR_2, bad_inside, bad_inside], [2, 2, 2], [2, 5], 2) == _want(3, 1, 2, 1, 2, 2, 3, 2)
    assert _score([FOR_2, FOR_2, FOR_2], [2, 2, 2], [2, 5], 2) == _want(3, 3, 3, 1, 2, 3, 3, 2)


def test_the_worst_class_is_found_by_cross_multiplication_and_ties_go_to_the_smaller_slot():
    for_7 = [0.0, 0.1, 0.9, 0.0]
    rows, exp = [FOR_5, for_7, for_7, FOR_5], [5, 5, 7, 7]               # vote 1: both classes 1 of 2
    sc, per = _score(rows, exp, [5, 7], 1, per_class=True)
    assert sc == _want(4, 2, 2, 2, 5, 1, 2, 2) and per.tolist() == [0, 1, 1, 0] and per.dtype == np.int64
    # class 7 at 2 of 4 is the same fraction: still class 5
    assert _score(rows + [for_7, FOR_5], exp + [7, 7], [5, 7], 1) == _want(6, 3, 3, 2, 5, 1, 2, 2)
    # class 7 at 2 of 5 is smaller than 1 of 2
    assert _score(rows + [for_7, FOR_5, FOR_5], exp + [7, 7, 7], [5, 7], 1) == _want(7, 3, 3, 2, 7, 2, 5, 2)


def test_a_subset_without_cue_rows():
    assert _score([FOR_2, FOR_5, FOR_5], [2, REST, 5], [9], 2) == _want(0, 0, 0, 0, -1, 0, 0, 1)
    assert _score([FOR_2], [2], [7, 9], 2) == _want(0, 0, 0, 0, -1, 0, 0, 2)       # no row is kept at all
    assert _score([], [], [2, 5], 25) == _want(0, 0, 0, 0, -1, 0, 0, 2)


def test_score_subset_refuses_what_it_cannot_score():
    from contrastiveprosthetics_amd.online import score_subset
    lg, exp = np.zeros((2, 4), dtype=np.float32), np.array([2, REST])
    for kw, what in ((dict(subset=[]), "empty"), (dict(subset=[3]), "not among ids"), (dict(subset=[2], vote=0), "vote"),
                     (dict(subset=[2], vote=257), "vote"), (dict(subset=[2], ids=[5, 2, 7, 9]), "ids"),
                     (dict(subset=[2], expected=np.array([2, 3])), "expected"), (dict(subset=[2], expected=exp[:1]), "expected")):
        a = dict(dict(logits=lg, expected=exp, ids=IDS, vote=25), **kw)
        with pytest.raises(ValueError, match=what):
            score_subset(a["logits"], a["expected"], a["ids"], a["subset"], vote=a["vote"])


def loop_reference(lg, exp, ids, subset, vote):
    """the sentences of the definition, row by row"""
    slot = {c: i for i, c in enumerate(ids)}
    S = sorted(slot[c] for c in subset)
    ring, n_c, hit_c, n_cue, hit = [], {}, {}, 0, 0
    for row, e in zip(lg, exp):
        e = int(e)
        if e >= 0 and slot[e] not in S:
            continue
        pred = -1
        if np.isfinite(row).all():
            for k in S:
                if pred < 0 or row[k] > row[pred]:
                    pred = k
        ring.append(pred)
        ring = ring[-vote:]
        voted, most = -1, 0
        for k in S:
            if ring.count(k) > most:
                voted, most = k, ring.count(k)
        if e >= 0:
            n_cue += 1
            hit += pred == slot[e]
            n_c[slot[e]] = n_c.get(slot[e], 0) + 1
            hit_c[slot[e]] = hit_c.get(slot[e], 0) + (voted == slot[e])
    worst = None
    for k in sorted(n_c):
        if worst is None or hit_c[k] * n_c[worst] < hit_c[worst] * n_c[k]:
            worst = k
    out = dict(n_cue=n_cue, hit=int(hit), voted_hit=sum(hit_c.values()), classes_scored=len(n_c),
               worst_class=-1 if worst is None else ids[worst], worst_hit=0 if worst is None else hit_c[worst],
               worst_n=0 if worst is None else n_c[worst], size=len(S))
    return out, [hit_c.get(k, 0) for k in range(len(ids))]


def test_score_subset_against_a_row_by_row_loop():
    from contrastiveprosthetics_amd.online import score_subset
    rng = np.random.default_rng(12)
    ids = [1, 3, 4, 8, 20, 21]
    seen = set()
    for trial in range(40):
        n = int(rng.integers(1, 120))
        lg = (rng.integers(-8, 9, (n, 6)) / 8).astype(np.float32)
        lg[rng.random(n) < 0.05, int(rng.integers(6))] = [np.nan, np.inf, -np.inf][trial % 3]
        exp = np.repeat(rng.choice([IGNORE, REST] + ids, n), rng.integers(1, 9, n))[:n]
        subset = [int(c) for c in rng.choice(ids, int(rng.integers(1, 7)), replace=False)]
        vote = int(rng.choice([1, 2, 5, 25, 256]))
        got, per = score_subset(lg, exp, ids, subset, vote=vote, per_class=True)
        want, want_per = loop_reference(lg, exp, ids, subset, vote)
        assert got == want and per.tolist() == want_per, (trial, subset, vote)
        seen.add((got["hit"] != got["voted_hit"], got["classes_scored"] == got["size"]))
    assert len(seen) == 4                                                # the vote matters, and so do classes without a cue


# ---------------------------------------------------------------------------------------------------------------------------
# rank_subsets
# ---------------------------------------------------------------------------------------------------------------------------
def _table(rows):
    base = dict(n_cue=100, hit=50, voted_hit=60, classes_scored=3, worst_class=1, worst_hit=10, worst_n=20, size=3)
    return {k: np.array([dict(base, **r)[k] for r in rows], dtype=np.int64) for k in base}


def test_rank_subsets_orders_by_every_key_in_turn():
    from contrastiveprosthetics_amd.online import rank_subsets
    rows = [dict(classes_scored=2, worst_hit=20, voted_hit=100, hit=100),    # 0: a class without a cue: behind all complete ones
            dict(),                                                          # 1: the base
            dict(worst_hit=11),                                              # 2: a better worst class
            dict(worst_hit=11, worst_n=22),                                  # 3: 11/22 is the base's 10/20 ...
            dict(voted_hit=61),                                              # 4: ... more voted hits
            dict(voted_hit=61, hit=51),                                      # 5: ... and more raw hits
            dict(),                                                          # 6: the base again: behind 1
            dict(classes_scored=2, worst_hit=20, voted_hit=100, hit=100, n_cue=200)]   # 7: incomplete, and half of 0's ratios
    order = rank_subsets(_table(rows))
    assert order.tolist() == [2, 5, 4, 1, 3, 6, 0, 7] and order.dtype == np.int64
    assert rank_subsets(_table([dict()] * 5)).tolist() == [0, 1, 2, 3, 4]   # all equal: the index
    # a subset without any cue row: every ratio is over max(., 1)
    none = dict(n_cue=0, hit=0, voted_hit=0, classes_scored=0, worst_class=-1, worst_hit=0, worst_n=0)
    assert rank_subsets(_table([none, dict(), dict(none, size=0)])).tolist() == [1, 2, 0]
    # the ratios, not the counts
    assert rank_subsets(_table([dict(worst_hit=30, worst_n=70), dict(worst_hit=3, worst_n=6)])).tolist() == [1, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# candidate generation (through a scoring callable: no device)
# ---------------------------------------------------------------------------------------------------------------------------
def fake_score(calls):
    """scores that depend on the mask alone: complete, and the better the larger (mask * 37) % 101 is"""
    def score(masks):
        from contrastiveprosthetics_amd.online import _mask_sizes
        assert masks.dtype == np.uint64 and masks.ndim == 1
        calls.append(masks.copy())
        size = _mask_sizes(masks)
        worth = (masks.astype(np.int64) * 37) % 101
        return dict(n_cue=np.full(size.shape, 200), hit=worth, voted_hit=worth, classes_scored=size,
                    worst_class=np.zeros_like(size), worst_hit=worth, worst_n=np.full(size.shape, 101), size=size)
    return score


def test_exhaustive_sizes_are_enumerated_completely_in_combinations_order():
    from contrastiveprosthetics_amd.online import _search_masks
    K, require = 7, (1 << 1) | (1 << 4)
    calls = []
    found = _search_masks(K, fake_score(calls), min_size=2, max_size=5, require=require, keep=3)
    assert [r["size"] for r in found] == [2, 3, 4, 5] and all(r["exhaustive"] is True for r in found)
    for r, masks in zip(found, calls):
        assert r["n_candidates"] == math.comb(K - 2, r["size"] - 2) == masks.shape[0]
        want = [sum(1 << i for i in c) for c in itertools.combinations(range(K), r["size"]) if 1 in c and 4 in c]
        assert masks.tolist() == want                                     # every one, in the order of combinations of slots
        assert len(r["best"]) == min(3, r["n_candidates"]) and all(m & require == require for m, _ in r["best"])
        worth = [(m * 37) % 101 for m in want]
        assert [m for m, _ in r["best"]] == [want[i] for i in sorted(range(len(want)), key=lambda i: (-worth[i], i))[:3]]
        assert all(tuple(sc) == KEYS + ("size",) and type(sc["hit"]) is int for _, sc in r["best"])
    # without require, and with the default max_size: every size up to K
    calls = []
    found = _search_masks(5, fake_score(calls), min_size=1)
    assert [r["n_candidates"] for r in found] == [5, 10, 10, 5, 1]


def test_beam_extensions_are_deduplicated_ordered_and_contain_require():
    from contrastiveprosthetics_amd.online import _search_masks
    K, require = 9, 1 << 3
    calls = []
    found = _search_masks(K, fake_score(calls), min_size=2, max_size=5, require=require, exhaustive=10, beam=4, keep=50)
    assert [r["exhaustive"] for r in found] == [True, False, False, False]       # 8, then C(8, 2) = 28 > 10
    for i in (1, 2, 3):
        prev = [m for m, _ in found[i - 1]["best"]][:4]                           # the best `beam` of the size before, in rank order
        want = sorted({m | 1 << b for m in prev for b in range(K) if not m >> b & 1})
        assert calls[i].tolist() == want and found[i]["n_candidates"] == len(want) < 4 * (K - found[i]["size"] + 1)
        assert all(m & require for m in want) and all(bin(m).count("1") == found[i]["size"] for m in want)
    # exhaustive=1 from the size of require on: one candidate, then extensions
    calls = []
    found = _search_masks(6, fake_score(calls), min_size=2, max_size=4, require=0b100010, exhaustive=1, beam=2)
    assert [(r["exhaustive"], r["n_candidates"]) for r in found] == [(True, 1), (False, 4), (False, 5)]
    # a size that is small enough again is enumerated again
    found = _search_masks(6, fake_score([]), min_size=1, exhaustive=6, beam=2)
    assert [r["exhaustive"] for r in found] == [True, False, False, False, True, True]
    assert [r["n_candidates"] for r in found][-2:] == [6, 1]


def test_candidates_reach_the_scorer_in_calls_of_at_most_the_maximum():
    from contrastiveprosthetics_amd.online import _search_masks
    calls, whole = [], []
    cut = _search_masks(6, fake_score(calls), min_size=3, max_size=3, max_call=7)
    assert [c.shape[0] for c in calls] == [7, 7, 6]
    assert cut == _search_masks(6, fake_score(whole), min_size=3, max_size=3)


def test_search_refuses_sizes_it_cannot_serve():
    from contrastiveprosthetics_amd.online import _search_masks
    score = fake_score([])
    for kw, what in ((dict(exhaustive=20), "no smaller size"), (dict(min_size=0), "min_size"), (dict(max_size=8), "max_size"),
                     (dict(min_size=4, max_size=3), "min_size <= max_size"), (dict(require=0b111), "required classes"),
                     (dict(beam=0), "beam"), (dict(keep=0), "keep"), (dict(exhaustive=0), "exhaustive"), (dict(beam=2.5), "beam")):
        with pytest.raises(ValueError, match=what):
            _search_masks(7, score, **dict(dict(min_size=2, max_size=4), **kw))  # (C(7, 2) = 21 > 20)


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper: what it refuses before the device is asked for anything, and what it hands over
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from contrastiveprosthetics_amd import online
    calls = []

    def stub(logits, slots, k, masks, vote, per_class):
        import torch
        calls.append((slots.copy(), k, masks.copy(), vote, per_class))
        scores = np.tile(np.array([9, 5, 6, 2, 1, 3, 4], dtype=np.int64), (masks.shape[0], 1))
        return scores, (torch.ones(masks.shape[0], 64, dtype=torch.int32) if per_class else None)

    monkeypatch.setattr(online, "_subsets_dev", stub)
    return calls


def test_sweep_subsets_refuses_bad_arguments_without_a_device_call(no_device):
    import torch
    from contrastiveprosthetics_amd.online import MAX_SUBSETS, search_grasp_sets, sweep_subsets
    lg, exp = torch.zeros(4, 4), np.array([REST, 5, 5, IGNORE])
    assert MAX_SUBSETS == 1048576
    bad = [(dict(subsets=[[2], [3]]), "subset 1 names 3"), (dict(subsets=[[2], []]), "subset 1 is empty"),
           (dict(subsets=[]), "1048576"), (dict(subsets=np.ones(MAX_SUBSETS + 1, dtype=np.uint64)), "1048576"),
           (dict(subsets=np.array([1, 16], dtype=np.uint64)), "subset 1 has a bit"),
           (dict(subsets=np.array([1, 0], dtype=np.uint64)), "subset 1 is empty"),
           (dict(subsets=np.ones((2, 2), dtype=np.uint64)), "uint64"), (dict(subsets=[[2.0]]), "not among ids"),
           (dict(vote=0), "vote"), (dict(vote=257), "vote"), (dict(vote=2.0), "vote"),
           (dict(expected=exp[:3]), "expected"), (dict(expected=np.array([0, 5, 5, 5])), "expected"),
           (dict(logits=torch.zeros(4, 3)), "logits"), (dict(logits=torch.zeros(4, 4, dtype=torch.float64)), "logits"),
           (dict(ids=[5, 2, 7, 9]), "ids"),
           (dict(), "GPU")]                                              # valid, but host logits: refused before the device
    for kw, what in bad:
        a = dict(dict(logits=lg, expected=exp, ids=IDS, subsets=[[2, 5]], vote=25), **kw)
        with pytest.raises(ValueError, match=re.escape(what)):
            sweep_subsets(a["logits"], a["expected"], a["ids"], a["subsets"], vote=a["vote"])
    with pytest.raises(ValueError, match="not among ids"):
        search_grasp_sets(lg, exp, IDS, require=[3])
    with pytest.raises(ValueError, match="expected"):
        search_grasp_sets(lg, exp[:2], IDS)
    assert no_device == []


def test_sweep_subsets_hands_the_device_slots_and_masks_and_maps_the_worst_class(no_device):
    import torch
    from contrastiveprosthetics_amd.online import sweep_subsets

    class OnDevice(torch.Tensor):                                        # host memory that says it is on the GPU
        @property
        def device(self):
            return torch.device("cuda:0")

    lg = torch.zeros(4, 4).as_subclass(OnDevice)
    out, hits = sweep_subsets(lg, np.array([REST, 5, 9, IGNORE]), IDS, [[9, 2], (5,), {2, 5, 7, 9}], vote=7, per_class=True)
    assert tuple(out) == KEYS + ("size",) and all(v.shape == (3,) and v.dtype == np.int64 for v in out.values())
    assert out["worst_class"].tolist() == [5, 5, 5] and out["size"].tolist() == [2, 1, 4] and out["n_cue"].tolist() == [9, 9, 9]
    assert hits.shape == (3, 4)                                          # the K columns of the 64
    (slots, k, masks, vote, per_class), = no_device
    assert slots.tolist() == [-1, 1, 3, -2] and slots.dtype == np.int32 and k == 4 and vote == 7 and per_class
    assert masks.tolist() == [0b1001, 0b0010, 0b1111] and masks.dtype == np.uint64
    same = sweep_subsets(lg, np.array([REST, 5, 9, IGNORE]), IDS, np.array([0b1001, 0b0010, 0b1111], dtype=np.uint64), vote=7)
    assert all(np.array_equal(same[key], out[key]) for key in out) and no_device[1][4] is False


def test_no_rows_give_the_definitions_answer_without_a_launch(no_device):
    import torch
    from contrastiveprosthetics_amd.online import score_subset, sweep_subsets
    out, hits = sweep_subsets(torch.zeros(0, 4), np.zeros(0, dtype=np.int64), IDS, [[2, 5], [9]], per_class=True)
    want = score_subset(np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.int64), IDS, [2, 5])
    assert {key: int(v[0]) for key, v in out.items()} == want and out["size"].tolist() == [2, 1]
    assert hits.shape == (2, 4) and not hits.any() and no_device == []


def test_search_grasp_sets_returns_ids_that_set_classes_takes(no_device, monkeypatch):
    import torch
    from contrastiveprosthetics_amd import online
    seen = []

    def table(logits, expected, ids, subsets, vote=25, per_class=False):
        seen.append((subsets.copy(), vote))
        return fake_score([])(subsets)

    monkeypatch.setattr(online, "sweep_subsets", table)
    found = online.search_grasp_sets(torch.zeros(3, 4), np.array([2, 5, REST]), IDS, min_size=2, max_size=3, vote=9, require=[7], keep=2)
    assert [r["size"] for r in found] == [2, 3] and [r["n_candidates"] for r in found] == [3, 3] and seen[0][1] == 9
    for r in found:
        for ids, sc in r["best"]:
            assert isinstance(ids, tuple) and 7 in ids and len(ids) == r["size"] == sc["size"] and list(ids) == sorted(ids)
            assert set(ids) <= set(IDS)
    assert seen[0][0].tolist() == [0b0101, 0b0110, 0b1100]


def test_subset_names_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    from contrastiveprosthetics_amd import online
    for n in ("SUBSET_SCORE_KEYS", "score_subset", "sweep_subsets", "rank_subsets", "search_grasp_sets"):
        assert getattr(pkg, n) is getattr(online, n), n


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_subset_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    assert set(_lib.SYMBOLS) == set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", hdr))   # the header's names are the binding's
    n_scores = int(re.search(r"#define\s+CP_ONLINE_SUBSET_SCORES\s+(\d+)", hdr).group(1))
    assert n_scores == _lib.CP_ONLINE_SUBSET_SCORES == len(KEYS) == 7
    n_max = int(re.search(r"#define\s+CP_ONLINE_SUBSET_SWEEP_MAX_SUBSETS\s+(\d+)", hdr).group(1))
    assert n_max == _lib.CP_ONLINE_SUBSET_SWEEP_MAX_SUBSETS == 1048576


def test_subset_scratch_is_sixty_four_bytes_per_row(lib):
    f = lib.cp_online_subset_sweep_scratch_bytes
    for n in (1, 3, 4, 5, 6000, 20500, 2 ** 31 - 1):
        assert 64 * n <= f(n) < 64 * n + 256 and f(n) % 256 == 0, n
    assert f(0) == f(1) == f(-3)


def test_subset_sweep_refuses_bad_arguments_before_any_device_call(lib):
    """host memory in every pointer: each refusal returns before a launch, which on this machine would fail differently"""
    M, K, G = 10, 5, 3
    lg = (ctypes.c_float * (M * 8))()
    exp = (ctypes.c_int32 * M)()
    masks = (ctypes.c_uint64 * G)(1, 3, 7)
    scores = (ctypes.c_int64 * (7 * G))()
    hits = (ctypes.c_int32 * (64 * G))()
    need = lib.cp_online_subset_sweep_scratch_bytes(M)
    buf = ctypes.create_string_buffer(need + 256)
    scratch = (ctypes.addressof(buf) + 255) // 256 * 256
    good = dict(logits=lg, ldl=8, n_rows=M, n_classes=K, expected=exp, subsets=masks, n_subsets=G, vote=25, scratch=scratch,
                scratch_bytes=need, scores=scores, class_hits=hits)

    def refused(what, **kw):
        a = dict(good, **kw)
        rc = lib.cp_online_subset_sweep(a["logits"], a["ldl"], a["n_rows"], a["n_classes"], a["expected"], a["subsets"],
                                        a["n_subsets"], a["vote"], a["scratch"], a["scratch_bytes"], a["scores"], a["class_hits"], None)
        assert rc == ERR_ARG, (kw, rc)
        msg = lib.cp_last_error()
        assert b"cp_online_subset_sweep" in msg and what.encode() in msg, (kw, msg)

    refused("n_classes", n_classes=0)
    refused("n_classes", n_classes=65)
    refused("ldl", n_classes=9)                                          # more classes than the rows are long
    refused("ldl", ldl=4)
    refused("n_subsets", n_subsets=0)
    refused("n_subsets", n_subsets=1048577)
    refused("vote", vote=0)
    refused("vote", vote=257)
    refused("n_rows", n_rows=0)
    refused("n_rows", n_rows=-5)
    refused("n_rows", n_rows=2 ** 31)
    refused("scratch", scratch_bytes=64 * M - 1)
    refused("scratch", scratch_bytes=0)
    refused("scratch", scratch=None)
    refused("logits", logits=None)
    refused("expected_slot", expected=None)
    refused("subsets", subsets=None)
    refused("scores", scores=None)
    refused("misaligned", scores=ctypes.addressof(scores) + 4)
    refused("misaligned", subsets=ctypes.addressof(masks) + 4)
    refused("misaligned", scratch=scratch + 8)
    refused("misaligned", class_hits=ctypes.addressof(hits) + 2)
