"""CPU checks of cue realignment (contrastiveprosthetics_amd/realign.py; csrc/online_realign.cuh): the definition against a
window-by-window loop in Python integers and Fractions, on planted two-level signals, ties, every status and the labelling
rules; `sample_labels` through `window_labels`; `activity_reference` at the edges of its rounding; the wrappers' refusals
through a stubbed device call; and the two C entries' declarations, constants and refusals before any device call."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ENTRIES = ["cp_online_realign_activity", "cp_online_realign"]
ERR_ARG = 10001
REST, IGNORE = -1, -2
DEFAULTS = dict(max_lag=100, max_lead=50, min_len=25, min_rest=10, context=100, min_contrast=0, guard=5)


def P(**kw):
    return dict(DEFAULTS, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# the sentences of the definition, pair by pair and window by window
# ---------------------------------------------------------------------------------------------------------------------------
def loop_pairs(a, s, e, r0, r1, p):
    """every pair inside the length limits of one region: (has the contrast, p / q as a Fraction, o, f, S_A, S_R)"""
    a = [min(max(int(v), 0), 4095) for v in a]
    L, T, out = r1 - r0, sum(a[r0:r1]), []
    for o in range(s, min(s + p["max_lag"], e - p["min_len"]) + 1):
        for f in range(max(o + p["min_len"], e - p["max_lead"]), r1 + 1):
            nA = f - o
            nR = L - nA
            if nR < p["min_rest"]:
                continue
            SA = sum(a[o:f])
            SR = T - SA
            has = SA * nR - SR * nA >= max(p["min_contrast"] * nA * nR, 1)
            out.append((has, Fraction(SA * SA * nR + SR * SR * nA, nA * nR), o, f, SA, SR))
    return out


def loop_reference(a, cue, segments, p):
    cue = [int(c) for c in cue]
    M, n, g = len(cue), len(segments), p["guard"]
    out = [c if c < 0 else IGNORE for c in cue]
    table, sums, ties = [], [], []
    for i, (s, e) in enumerate((int(s), int(e)) for s, e in segments):
        prev_e = int(segments[i - 1][1]) if i else 0
        next_s = int(segments[i + 1][0]) if i + 1 < n else M
        ties.append(0)
        if not (0 <= s < e <= M) or s < prev_e:
            table.append((s, e, -1, -1, -1, -1, 4, -1))
            sums.append((0, 0))
            continue
        r0 = max(s - p["context"], prev_e, 0)
        r1 = min(e + p["max_lag"], max(next_s, e), M)
        if r1 - r0 > 4096:
            table.append((s, e, r0, r1, -1, -1, 3, cue[s]))
            sums.append((0, 0))
            continue
        pairs = loop_pairs(a, s, e, r0, r1, p)
        if not pairs:
            table.append((s, e, r0, r1, -1, -1, 1, cue[s]))
            sums.append((0, 0))
            continue
        found = any(x[0] for x in pairs)
        pool = [x for x in pairs if x[0] == found]
        top = max(x[1] for x in pool)
        best = sorted((x[2], x[3], x[4], x[5]) for x in pool if x[1] == top)
        ties[-1] = len(best)
        o, f, SA, SR = best[0]
        table.append((s, e, r0, r1, o, f, 0 if found else 2, cue[s]))
        sums.append((SA, SR))
        if not found:
            continue
        for k in range(s, r1):
            if o + g <= k < f - g:
                out[k] = cue[s]
            elif k < e:
                out[k] = REST if (k < o - g or k >= f + g) else IGNORE
            else:
                out[k] = IGNORE if k < f + g else cue[k]
    return np.array(out, dtype=np.int64), np.array(table, dtype=np.int32).reshape(n, 8), np.array(sums, dtype=np.int64).reshape(n, 2), ties


def same_as_loop(a, cue, segments, p):
    from contrastiveprosthetics_amd.realign import realign_reference
    got = realign_reference(a, cue, segments, **p)
    want = loop_reference(a, cue, segments, p)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    for g, w, what in zip(got, want, ("expected", "table", "sums")):
        assert np.array_equal(g, w), (what, g, w)
    return got, want[3]


def cued_recording(rng, M, n_seg, step=(300, 700), noise=200, lag=(0, 40), over=(-15, 30)):
    """a cue of n_seg segments in M windows (starts and ends at drawn multiples of 10) and a noisy two-level activity behind it"""
    cuts = np.sort(rng.choice(np.arange(1, M // 10), 2 * n_seg, replace=False)) * 10
    cue = np.full(M, REST, dtype=np.int64)
    a = rng.integers(0, noise + 1, M)
    for i in range(n_seg):
        s, e = int(cuts[2 * i]), int(cuts[2 * i + 1])
        cue[s:e] = int(rng.integers(0, 5))
        o = s + int(rng.integers(lag[0], lag[1] + 1))
        f = min(max(e + int(rng.integers(over[0], over[1] + 1)), o + 1), M)
        a[o:f] += rng.integers(step[0], step[1] + 1, max(f - o, 0))
    return a, cue


# ---------------------------------------------------------------------------------------------------------------------------
# 1. planted pairs
# ---------------------------------------------------------------------------------------------------------------------------
def test_noise_free_two_level_signals_give_the_planted_pair_exactly():
    from contrastiveprosthetics_amd.realign import cue_segments, realign_reference
    rng = np.random.default_rng(0)
    for trial in range(60):
        M = 700
        cue = np.full(M, REST)
        s = int(rng.integers(120, 200))
        e = s + int(rng.integers(150, 400))
        cue[s:e] = 3
        o, f = s + int(rng.integers(0, 90)), min(e + int(rng.integers(-40, 90)), M)       # early or late release
        a = np.full(M, int(rng.integers(0, 300)))
        a[o:f] += int(rng.integers(50, 2500))
        seg = cue_segments(cue)
        assert seg.tolist() == [[s, e]] and seg.dtype == np.int32
        exp, table, sums = realign_reference(a, cue, seg, **DEFAULTS)
        assert table[0].tolist() == [s, e, max(s - 100, 0), min(e + 100, M), o, f, 0, 3], (trial, table)
        assert sums[0].tolist() == [int(a[o:f].sum()), int(a[max(s - 100, 0):min(e + 100, M)].sum() - a[o:f].sum())]


def test_the_definition_against_the_loop_on_noisy_recordings():
    rng = np.random.default_rng(1)
    from contrastiveprosthetics_amd.realign import cue_segments
    seen = set()
    for trial in range(12):
        M = int(rng.integers(300, 600))
        a, cue = cued_recording(rng, M, int(rng.integers(1, 5)), noise=int(rng.choice([0, 50, 400])))
        p = P(max_lag=int(rng.choice([0, 20, 60])), max_lead=int(rng.choice([0, 10, 40])), context=int(rng.choice([0, 30, 100])),
              min_len=int(rng.choice([1, 11, 25])), min_rest=int(rng.choice([1, 10, 40])), guard=int(rng.choice([0, 5])),
              min_contrast=int(rng.choice([0, 0, 450])))
        p["min_len"] = max(p["min_len"], 2 * p["guard"] + 1)
        (exp, table, sums), _ = same_as_loop(a, cue, cue_segments(cue), p)
        seen |= set(table[:, 6].tolist())
    assert {0, 2} <= seen


def test_cue_segments_are_the_runs_of_score_commands():
    from contrastiveprosthetics_amd.realign import cue_segments
    cue = np.array([3, 3, REST, 4, 4, 5, IGNORE, 5, 5, REST, REST, 0])
    assert cue_segments(cue).tolist() == [[0, 2], [3, 5], [5, 6], [7, 9], [11, 12]]
    assert cue_segments(np.array([REST, IGNORE])).shape == (0, 2) and cue_segments(np.zeros(0, dtype=np.int64)).shape == (0, 2)
    assert cue_segments(np.array([7])).tolist() == [[0, 1]]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. ties
# ---------------------------------------------------------------------------------------------------------------------------
def tie_case():
    """a burst of 12 windows under min_len 20: the 8 windows of rest a pair must take along can lie in front or behind"""
    M = 200
    cue = np.full(M, REST)
    cue[50:130] = 2
    a = np.zeros(M, dtype=np.int64)
    a[80:92] = 500
    return a, cue, P(max_lag=60, max_lead=60, min_len=20, min_rest=10, context=30, guard=2)


def test_equal_fractions_go_to_the_smaller_onset_then_the_smaller_offset():
    from contrastiveprosthetics_amd.realign import cue_segments
    a, cue, p = tie_case()
    (exp, table, sums), ties = same_as_loop(a, cue, cue_segments(cue), p)
    assert ties[0] > 1                                                    # the data has a tie: several pairs at the largest p / q
    pairs = loop_pairs(a, 50, 130, 20, 190, p)
    top = max(x[1] for x in pairs if x[0])
    equal = sorted((x[2], x[3]) for x in pairs if x[0] and x[1] == top)
    assert len(equal) == ties[0] and len({o for o, _ in equal}) > 1       # and they differ in the onset
    assert table[0, 4:7].tolist() == [equal[0][0], equal[0][1], 0] and equal[0] == (72, 92)
    # constant activity: every pair has the same p / q = c^2 L, none has the contrast: the first onset and its first offset
    flat = np.full(200, 7)
    (exp, table, sums), ties = same_as_loop(flat, cue, cue_segments(cue), p)
    assert ties[0] == len(pairs) and table[0, 4:7].tolist() == [50, 70, 2] and (exp[50:130] == IGNORE).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the other statuses
# ---------------------------------------------------------------------------------------------------------------------------
def test_status_1_2_and_3():
    from contrastiveprosthetics_amd.realign import cue_segments, realign_reference
    M = 300
    cue = np.full(M, REST)
    cue[100:120] = 1                                                     # 20 windows under min_len 25
    a = np.zeros(M, dtype=np.int64)
    a[105:118] = 900
    exp, table, sums = realign_reference(a, cue, cue_segments(cue), **DEFAULTS)
    assert table[0].tolist() == [100, 120, 0, 220, -1, -1, 1, 1] and sums[0].tolist() == [0, 0]
    assert (exp[100:120] == IGNORE).all() and (exp[:100] == REST).all() and (exp[120:] == REST).all()
    # min_rest out of reach: the region is 60 windows and a pair takes 25 at least
    cue = np.full(60, REST)
    cue[10:50] = 1
    exp, table, sums = realign_reference(np.arange(60), cue, cue_segments(cue), **P(min_rest=36))
    assert table[0, 6] == 1
    assert realign_reference(np.arange(60), cue, cue_segments(cue), **P(min_rest=35))[1][0, 6] == 0
    # a dip instead of a rise
    cue = np.full(M, REST)
    cue[100:200] = 4
    a = np.full(M, 800)
    a[110:] = 100                                                        # (a pair holds 10 windows of the high level at most)
    (exp, table, sums), _ = same_as_loop(a, cue, cue_segments(cue), DEFAULTS)
    assert table[0, 6] == 2 and table[0, 4] >= 100 and table[0, 5] > table[0, 4] and (exp[100:200] == IGNORE).all()
    assert sums[0, 0] == a[table[0, 4]:table[0, 5]].sum()
    # a rise that min_contrast does not accept
    a = np.full(M, 100)
    a[120:190] = 300
    assert realign_reference(a, cue, cue_segments(cue), **P(min_contrast=200))[1][0, 4:7].tolist() == [120, 190, 0]
    assert realign_reference(a, cue, cue_segments(cue), **P(min_contrast=201))[1][0, 6] == 2
    # L = 4096 is a region, 4097 is not
    M = 5000
    a = np.random.default_rng(3).integers(0, 50, M)
    a[300:4000] += 2000
    for e, status in ((10 + 4096, 0), (10 + 4097, 3)):
        cue = np.full(M, REST)
        cue[10:e] = 0
        exp, table, sums = realign_reference(a, cue, cue_segments(cue), **P(context=0, max_lag=0, max_lead=200))
        assert table[0, :4].tolist() == [10, e, 10, e] and table[0, 6] == status and table[0, 7] == 0
        assert (table[0, 4] == 10 and table[0, 5] == 4000) if status == 0 else (table[0, 4] == table[0, 5] == -1)
        assert (exp[10:e] == IGNORE).all() if status else (exp[15:3995] == 0).all()


def test_bad_table_rows_have_status_4_and_touch_nothing():
    rng = np.random.default_rng(5)
    M = 400
    a, cue = cued_recording(rng, M, 3)
    rows = [[20, 60], [90, 80], [100, 150], [140, 170], [200, 401], [-3, 10], [300, 340]]
    (exp, table, sums), _ = same_as_loop(a, cue, np.array(rows), P(max_lag=30, context=30))
    assert table[:, 6].tolist()[1] == 4 and table[3, 6] == 4 and table[4, 6] == 4 and table[5, 6] == 4
    assert table[0, 6] != 4 and table[2, 6] != 4 and table[6, 6] != 4
    assert table[1].tolist() == [90, 80, -1, -1, -1, -1, 4, -1]


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the labels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", [0, 5])
def test_the_labels_of_a_found_segment(guard):
    from contrastiveprosthetics_amd.realign import cue_segments, realign_reference
    M = 400
    cue = np.full(M, REST)
    cue[100:200] = 6
    cue[260:265] = IGNORE
    for o, f in ((130, 180), (130, 230)):                                # an early release and a late one
        a = np.zeros(M, dtype=np.int64)
        a[o:f] = 1000
        exp, table, sums = realign_reference(a, cue, cue_segments(cue), **P(guard=guard))
        assert table[0].tolist() == [100, 200, 0, 300, o, f, 0, 6]
        want = cue.copy()
        want[100:200] = REST
        want[o - guard:f + guard] = IGNORE
        want[o + guard:f - guard] = 6
        assert np.array_equal(exp, want), (o, f, np.nonzero(exp != want))
        assert exp[260] == IGNORE and exp[299] == REST


def test_back_to_back_segments_a_segment_at_window_0_and_one_ending_at_m():
    from contrastiveprosthetics_amd.realign import cue_segments
    M = 500
    cue = np.full(M, REST)
    cue[0:100], cue[100:200], cue[230:330], cue[400:500] = 1, 2, 3, 4     # gap 0, a gap of 30 < max_lag, the end at M
    a = np.zeros(M, dtype=np.int64)
    for o, f in ((20, 100), (125, 215), (255, 360), (430, 500)):
        a[o:f] = 700
    a += np.random.default_rng(7).integers(0, 60, M)
    (exp, table, sums), _ = same_as_loop(a, cue, cue_segments(cue), DEFAULTS)
    assert table[:, 6].tolist() == [0, 0, 0, 0] and table[:, 7].tolist() == [1, 2, 3, 4]
    assert table[:, 2].tolist() == [0, 100, 200, 330] and table[:, 3].tolist() == [100, 230, 400, 500]
    assert (table[:-1, 5] <= table[1:, 0]).all() and (table[:-1, 3] <= table[1:, 0]).all()       # offset_i <= s_{i+1}: no overlap
    assert np.abs(table[:, 4] - [20, 125, 255, 430]).max() <= 1 and np.abs(table[:, 5] - [100, 215, 360, 500]).max() <= 1
    assert exp[0] == REST and exp[table[3, 5] - 5] == IGNORE and exp[table[3, 5] - 6] == 4 and exp[50] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# 5. sample_labels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 7])
def test_sample_labels_round_trip_through_window_labels(phase):
    from contrastiveprosthetics_amd import online
    from contrastiveprosthetics_amd.realign import sample_labels
    assert (online.REST, online.IGNORE, online.STRIDE) == (REST, IGNORE, 20)
    rng = np.random.default_rng(phase)
    for n in (0, 10, phase + 11, 2000, 2013):
        k = online.windows_before(n, phase)
        x = np.repeat(rng.choice([REST, IGNORE, 0, 3, 9], k), rng.integers(1, 6, k))[:k].astype(np.int64)
        lab = sample_labels(x, n, phase, rest=17)
        assert lab.shape == (n,) and lab.dtype == np.int64 and (lab[:phase] == -1).all()
        assert np.array_equal(online.window_labels(lab, phase), np.where(x == REST, 17, np.where(x == IGNORE, -1, x)))
        assert np.array_equal(online.expected_commands(lab, [0, 3, 9], phase, rest=17), x)
        for j in range(min(k, 5)):
            block = lab[phase + 20 * j:phase + 20 * j + 20]
            assert (block == (17 if x[j] == REST else -1 if x[j] == IGNORE else x[j])).all()
        none = sample_labels(x, n, phase)
        assert np.array_equal(none, np.where(lab == 17, -1, lab))           # without a rest label REST is not labelled


# ---------------------------------------------------------------------------------------------------------------------------
# 6. activity
# ---------------------------------------------------------------------------------------------------------------------------
def test_activity_reference_at_the_edges_of_its_rounding():
    from contrastiveprosthetics_amd.realign import activity_reference
    nan, inf = float("nan"), float("inf")
    one = lambda v, base=0.0, gain=1.0: int(activity_reference(np.array([[v] + [0.0] * 11], dtype=np.float32),  # noqa: E731
                                                               [base] + [0.0] * 11, [gain] + [1.0] * 11)[0])
    for v, want in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4), (254.5, 254), (255.5, 255), (254.49, 254), (1e9, 255), (-0.5, 0), (-3.0, 0),
                    (nan, 0), (inf, 255), (-inf, 0), (0.50001, 1)):
        assert one(v) == want, v
    assert one(inf, gain=0.0) == 0 and one(inf, base=inf) == 0 and one(5.0, gain=nan) == 0 and one(7.0, gain=0.0) == 0
    assert one(10.5, base=10.0, gain=3.0) == 2 and one(10.5, base=10.0, gain=5.0) == 2 and one(10.5, base=10.0, gain=7.0) == 4
    full = activity_reference(np.full((3, 12), 1e6, dtype=np.float32), np.zeros(12), np.ones(12))
    assert full.tolist() == [3060] * 3 and full.dtype == np.int32
    # float32 operations, not float64 ones: 16777217 is not a float32
    assert one(16777217.0, base=16777216.0, gain=1.0) == 0


def test_activity_profile():
    from contrastiveprosthetics_amd.realign import activity_profile
    rng = np.random.default_rng(11)
    M = 600
    cue = np.full(M, REST)
    cue[200:300] = 2
    cue[590:] = IGNORE
    w = rng.normal(0, 1, (M, 12)).astype(np.float32)
    w[200:330] += 6.0                                                    # the hand lets go 30 windows late
    w[:, 3] = 2.0                                                        # a channel that does nothing
    prof = activity_profile(w, cue, level=0.9, settle=50)
    settled = np.r_[0:200, 349:590]
    assert np.array_equal(prof["base"], np.median(w[settled].astype(np.float64), axis=0).astype(np.float32))
    span = np.quantile(w[200:300].astype(np.float64), 0.9, axis=0) - np.median(w[settled].astype(np.float64), axis=0)
    span[3] = 1.0
    assert prof["gain"][3] == 0 and np.array_equal(np.delete(prof["gain"], 3), np.delete((255.0 / span).astype(np.float32), 3))
    assert prof["base"].dtype == prof["gain"].dtype == np.float32
    # no REST window is far enough behind a cue: all of them
    late = np.full(40, REST)
    late[:10] = 1
    assert np.array_equal(activity_profile(w[:40], late, settle=100)["base"], np.median(w[10:40].astype(np.float64), axis=0).astype(np.float32))
    for kw, what in ((dict(cue=np.zeros(M, dtype=np.int64)), "REST"), (dict(level=0.0), "level"), (dict(level=1.5), "level"),
                     (dict(settle=-1), "settle"), (dict(settle=2.5), "settle"), (dict(cue=cue[:-1]), "go together"),
                     (dict(windows=w[:, :11]), "go together"), (dict(cue=cue.astype(np.float64)), "integer")):
        args = dict(dict(windows=w, cue=cue, level=0.95, settle=100), **kw)
        with pytest.raises(ValueError, match=what):
            activity_profile(args["windows"], args["cue"], level=args["level"], settle=args["settle"])


# ---------------------------------------------------------------------------------------------------------------------------
# a region whose products need their 128 bits (also built by tests/test_gpu_online_realign.py)
# ---------------------------------------------------------------------------------------------------------------------------
def truncated_choice(a, s, e, r0, r1, p):
    """the choice of a comparison that keeps the low 64 bits of p1 q2 and p2 q1, pairs in ascending (o, f)"""
    mask = (1 << 64) - 1
    Pf = np.concatenate([[0], np.cumsum(np.clip(a[r0:r1], 0, 4095))]).tolist()
    L, T, best = r1 - r0, Pf[-1], None
    for o in range(s, min(s + p["max_lag"], e - p["min_len"]) + 1):
        for f in range(max(o + p["min_len"], e - p["max_lead"]), min(r1, o + L - p["min_rest"]) + 1):
            nA = f - o
            nR = L - nA
            SA = Pf[f - r0] - Pf[o - r0]
            SR = T - SA
            if SA * nR - SR * nA < max(p["min_contrast"] * nA * nR, 1):
                continue
            pp, q = SA * SA * nR + SR * SR * nA, nA * nR
            if best is None or (pp * best[1]) & mask > (best[0] * q) & mask:
                best = (pp, q, o, f)
    return best[2], best[3], best[0].bit_length()


def long_region_case(seed=0):
    """s = 100, e = 3,900 in a region of 3,996 windows at activity 2,400..3,060: p has some 58 bits and q some 22, and the test
    asserts that a comparison cut to 64 bits picks another pair than the exact one"""
    from contrastiveprosthetics_amd.realign import cue_segments, realign_reference
    rng = np.random.default_rng(seed)
    M, s, e = 4300, 100, 3900
    cue = np.full(M, REST)
    cue[s:e] = 0
    a = rng.integers(2400, 3061, M)
    a[:s + 40] = rng.integers(0, 40, s + 40)
    a[e + 30:] = rng.integers(0, 40, M - e - 30)
    p = P(max_lag=96, max_lead=16)
    exp, table, sums = realign_reference(a, cue, cue_segments(cue), **p)
    assert table[0, :4].tolist() == [100, 3900, 0, 3996] and table[0, 6] == 0
    o, f, bits = truncated_choice(a, s, e, 0, 3996, p)
    assert bits > 50 and (o, f) != (int(table[0, 4]), int(table[0, 5])), (o, f, table[0])
    return a, cue, p, (exp, table, sums)


def test_a_comparison_cut_to_64_bits_picks_another_pair_in_a_long_high_region():
    a, cue, p, (exp, table, sums) = long_region_case()
    assert table[0, 4:6].tolist() == [140, 3930]                          # the planted pair


# ---------------------------------------------------------------------------------------------------------------------------
# the end-to-end recording of tests/test_gpu_online_realign.py, checked here with the oracle's windows
# ---------------------------------------------------------------------------------------------------------------------------
E2E_IDS, E2E_REST = [3, 8], 40


def stepped_recording(seed=4):
    """raw (n, 12) f32 noise whose amplitude steps x4 at planted sample positions, the cue as one label per sample (E2E_REST
    between the cues), and per segment the planted (lag, overrun) in windows: the lag is 30 windows at least"""
    rng = np.random.default_rng(seed)
    n = 20 * 1000 + 11
    labels = np.full(n, E2E_REST)
    raw = rng.standard_normal((n, 12)) * 1e-3
    amp, planted = np.ones(n), []
    for s, e, c in ((150, 300, 3), (450, 600, 8), (750, 900, 3)):
        labels[20 * s:20 * e] = c
        lag, over = int(rng.integers(30, 61)), int(rng.integers(-10, 41))
        amp[20 * (s + lag):20 * (e + over)] = 4.0
        planted.append((lag, over))
    return (raw * amp[:, None]).astype(np.float32), labels, planted


def lags_nearer_to_the_planted_ones_than_to_zero(segments, planted):
    lag = np.asarray(segments["lag"])
    want = np.array([p[0] for p in planted])
    return (np.asarray(segments["status"]) == 0).all() and (want >= 30).all() and (np.abs(lag - want) < np.abs(lag)).all()


def test_the_end_to_end_recording_meets_its_condition_with_the_oracles_windows(no_device):
    import torch
    from contrastiveprosthetics_amd.online import expected_commands
    from contrastiveprosthetics_amd.realign import realign_cues
    from oracle import preprocess_cpu as pc
    raw, labels, planted = stepped_recording()
    b, a = pc.butter_bandpass()
    y = pc.lfilter_df2t(b, a, raw * np.float32(pc.GAIN)).astype(np.float32)
    w = np.sqrt(pc.uniform_filter1d_nearest(np.square(y), pc.RMS_WINDOW))[pc.WINDOW_EDGE:-pc.WINDOW_EDGE][::20].astype(np.float32)
    w = ((w - w.mean(0)) / w.std(0)).astype(np.float32)
    cue = expected_commands(labels, E2E_IDS, 0, rest=E2E_REST)
    out = realign_cues(on_device(torch.from_numpy(w)), cue)               # (the stub: the definition on these windows)
    assert out["segments"]["start"].tolist() == [150, 450, 750] and out["segments"]["end"].tolist() == [300, 600, 900]
    assert lags_nearer_to_the_planted_ones_than_to_zero(out["segments"], planted)
    assert np.abs(out["segments"]["lag"] - [p[0] for p in planted]).max() <= 2       # (far inside the condition)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the wrappers: what they refuse before the device is asked for anything, and what they hand over
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from contrastiveprosthetics_amd import realign
    calls = []

    def stub(windows, activity, cue32, segments, cfg, base, gain, device):
        calls.append(dict(windows=windows, activity=activity, cue=cue32.copy(), segments=segments.copy(), cfg=dict(cfg), base=base,
                          gain=gain, device=device))
        act = realign.activity_reference(windows, base, gain) if activity is None else activity
        exp, table, sums = realign.realign_reference(act, cue32, segments, **cfg)
        return exp.astype(np.int32), table, sums

    monkeypatch.setattr(realign, "_realign_dev", stub)
    return calls


def on_device(t):
    import torch

    class OnDevice(torch.Tensor):                                        # host memory that says it is on the GPU
        @property
        def device(self):
            return torch.device("cuda:0")

    return t.as_subclass(OnDevice)


def test_realign_cues_refuses_bad_arguments_without_a_device_call(no_device):
    import torch
    from contrastiveprosthetics_amd.realign import realign_cues
    M = 300
    cue = np.full(M, REST)
    cue[100:200] = 1
    w = on_device(torch.zeros(M, 12))
    prof = dict(base=np.zeros(12, dtype=np.float32), gain=np.ones(12, dtype=np.float32))
    bad = [(dict(max_lag=-1), "max_lag"), (dict(max_lag=1025), "max_lag"), (dict(max_lead=-1), "max_lead"), (dict(max_lead=1025), "max_lead"),
           (dict(context=-1), "context"), (dict(context=2049), "context"), (dict(min_len=0), "min_len"), (dict(min_rest=0), "min_rest"),
           (dict(guard=-1), "guard"), (dict(guard=13), "guard"), (dict(guard=12, min_len=24), "guard"), (dict(min_contrast=-1), "min_contrast"),
           (dict(min_contrast=4096), "min_contrast"), (dict(max_lag=2.0), "max_lag"), (dict(guard=True), "guard"),
           (dict(cue=cue[:-1]), "one entry per window"), (dict(cue=cue.astype(np.float32)), "integer"), (dict(cue=cue.reshape(2, -1)), "1-d"),
           (dict(cue=np.zeros(0, dtype=np.int64), windows=on_device(torch.zeros(0, 12))), "one window"),
           (dict(cue=np.where(cue == 1, 2 ** 31, cue)), "32 bits"),
           (dict(windows=torch.zeros(M, 12)), "GPU"), (dict(windows=on_device(torch.zeros(M, 11))), "float32 tensor"),
           (dict(windows=on_device(torch.zeros(M, 12, dtype=torch.float64))), "float32 tensor"), (dict(windows=np.zeros((M, 12))), "float32 tensor"),
           (dict(windows=None), "float32 tensor"),
           (dict(profile=dict(base=np.zeros(12))), "profile"), (dict(profile=dict(base=np.zeros(12), gain=np.zeros(11))), "profile"),
           (dict(profile=3), "profile"),
           (dict(activity=np.zeros(M - 1, dtype=np.int64)), "activity"), (dict(activity=np.zeros(M)), "activity"),
           (dict(activity=np.zeros((M, 1), dtype=np.int64)), "activity"),
           (dict(cue=np.arange(2 * 65537) % 2 * 3 - 1, windows=None, activity=np.zeros(2 * 65537, dtype=np.int64)), "65536")]
    for kw, what in bad:
        a = dict(dict(windows=w, cue=cue, profile=prof, activity=None), **kw)
        with pytest.raises(ValueError, match=re.escape(what)):
            realign_cues(a.pop("windows"), a.pop("cue"), a.pop("profile"), **a)
    # the profile is made from the recording if none is given, and a recording without REST windows is refused there
    with pytest.raises(ValueError, match="REST"):
        realign_cues(w, np.where(cue == REST, IGNORE, cue))
    assert no_device == []


def test_realign_cues_hands_the_device_the_segments_and_names_the_columns(no_device):
    import torch
    from contrastiveprosthetics_amd.realign import SEGMENT_COLUMNS, activity_profile, realign_cues, realign_reference, activity_reference
    rng = np.random.default_rng(2)
    M = 500
    cue = np.full(M, REST)
    cue[100:200], cue[300:320] = 4, 2                                    # the second is shorter than min_len
    x = rng.normal(0, 1, (M, 12)).astype(np.float32)
    x[130:220] += 5.0
    w = on_device(torch.from_numpy(x))
    out = realign_cues(w, cue, min_rest=12)
    call, = no_device
    assert call["segments"].tolist() == [[100, 200], [300, 320]] and call["cue"].dtype == np.int32 and call["activity"] is None
    assert call["cfg"] == P(min_rest=12) and str(call["device"]) == "cuda:0"
    prof = activity_profile(x, cue)
    assert np.array_equal(call["base"], prof["base"]) and np.array_equal(call["gain"], prof["gain"])
    exp, table, sums = realign_reference(activity_reference(x, prof["base"], prof["gain"]), cue, call["segments"], **P(min_rest=12))
    assert set(out) == {"expected", "segments", "contrast"} and tuple(out["segments"]) == SEGMENT_COLUMNS
    assert out["expected"].dtype == np.int64 and np.array_equal(out["expected"], exp)
    seg = out["segments"]
    assert all(v.dtype == np.int64 and v.shape == (2,) for v in seg.values())
    assert seg["start"].tolist() == [100, 300] and seg["end"].tolist() == [200, 320] and seg["status"].tolist() == [0, 1]
    assert seg["cls"].tolist() == [4, 2] and seg["onset"][1] == seg["offset"][1] == -1 and seg["lag"][1] == seg["overrun"][1] == 0
    assert abs(seg["lag"][0] - 30) <= 2 and abs(seg["overrun"][0] - 20) <= 2 and seg["onset"][0] == 100 + seg["lag"][0]
    nA = seg["offset"][0] - seg["onset"][0]
    assert out["contrast"][0] == sums[0, 0] / nA - sums[0, 1] / (table[0, 3] - table[0, 2] - nA) and np.isnan(out["contrast"][1])
    # a caller's activity: no windows, clamped on the way
    act = np.where((np.arange(M) >= 130) & (np.arange(M) < 220), 9000, -5)
    out = realign_cues(None, cue, activity=act, guard=0)
    assert no_device[1]["windows"] is None and no_device[1]["activity"].min() == 0 and no_device[1]["activity"].max() == 4095
    assert out["segments"]["onset"][0] == 130 and out["segments"]["offset"][0] == 220
    # no segment at all: the definition's answer without a launch
    out = realign_cues(None, np.array([REST, IGNORE, REST]), activity=np.zeros(3, dtype=np.int64))
    assert out["expected"].tolist() == [REST, IGNORE, REST] and out["contrast"].shape == (0,) and len(no_device) == 2
    assert all(v.shape == (0,) for v in out["segments"].values())


def test_reference_and_sample_labels_refuse_what_they_cannot_take():
    from contrastiveprosthetics_amd.realign import activity_reference, cue_segments, realign_reference, sample_labels
    cue = np.array([REST] * 30 + [1] * 60 + [REST] * 30)
    a = np.zeros(120, dtype=np.int64)
    for kw, what in ((dict(min_len=10, guard=5), "guard"), (dict(max_lag=1025), "max_lag"), (dict(min_rest=0), "min_rest")):
        with pytest.raises(ValueError, match=what):
            realign_reference(a, cue, cue_segments(cue), **P(**kw))
    with pytest.raises(ValueError, match="segments"):
        realign_reference(a, cue, np.zeros((2, 3), dtype=np.int64), **DEFAULTS)
    with pytest.raises(ValueError, match="activity"):
        realign_reference(a[:-1], cue, cue_segments(cue), **DEFAULTS)
    with pytest.raises(ValueError, match="go together"):
        activity_reference(np.zeros((4, 11)), np.zeros(12), np.zeros(12))
    x = np.array([REST, 3, IGNORE])
    for args, what in (((x, 50), "2 windows"), ((x, 70, 20), "phase"), ((x, 70, -1), "phase"), ((x, -1), "n_samples"), ((x, 70, 0, -2), "rest"),
                       ((np.array([0, -3, 1]), 70), "class ids"), ((x.astype(np.float64), 70), "integer"), ((x, 70.0), "n_samples")):
        with pytest.raises(ValueError, match=what):
            sample_labels(*args)
    assert sample_labels(x, 70, 0, 8).tolist() == [8] * 20 + [3] * 20 + [-1] * 30


def test_realign_names_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    from contrastiveprosthetics_amd import realign
    for n in ("realign_cues", "realign_reference", "activity_profile", "activity_reference", "cue_segments", "sample_labels"):
        assert getattr(pkg, n) is getattr(realign, n), n


# ---------------------------------------------------------------------------------------------------------------------------
# 8. and 9. the C entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_realign_symbols_declared_exported_and_bound_and_constants_agree(lib):
    from contrastiveprosthetics_amd import _lib, realign
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    top = int(re.search(r"#define\s+CP_ONLINE_REALIGN_MAX_ACTIVITY\s+(\d+)", hdr).group(1))
    assert top == _lib.CP_ONLINE_REALIGN_MAX_ACTIVITY == realign.MAX_ACTIVITY == 4095
    region = int(re.search(r"#define\s+CP_ONLINE_REALIGN_MAX_REGION\s+(\d+)", hdr).group(1))
    assert region == _lib.CP_ONLINE_REALIGN_MAX_REGION == realign.MAX_REGION == 4096
    body = hdr[hdr.index("typedef struct cp_online_realign_config {"):hdr.index("} cp_online_realign_config;")]
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [f[0] for f in _lib.cp_online_realign_config._fields_] == list(realign._PARAMS)
    assert ctypes.sizeof(_lib.cp_online_realign_config) == 28


def test_realign_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory in every pointer: each refusal returns before a launch, which on this machine would fail differently"""
    from contrastiveprosthetics_amd import _lib
    M, N = 50, 3
    w = (ctypes.c_float * (M * 16))()
    base, gain = (ctypes.c_float * 12)(), (ctypes.c_float * 12)()
    act, cue, exp = (ctypes.c_int32 * M)(), (ctypes.c_int32 * M)(), (ctypes.c_int32 * M)()
    seg, table, sums = (ctypes.c_int32 * (2 * N))(), (ctypes.c_int32 * (8 * N))(), (ctypes.c_int64 * (2 * N))()
    addr = ctypes.addressof

    def activity_refused(what, **kw):
        a = dict(dict(windows=w, ldw=16, n_rows=M, base=base, gain=gain, activity=act), **kw)
        for k in ("base", "gain"):
            if isinstance(a[k], int):
                a[k] = ctypes.cast(a[k], ctypes.POINTER(ctypes.c_float))
        rc = lib.cp_online_realign_activity(a["windows"], a["ldw"], a["n_rows"], a["base"], a["gain"], a["activity"], None)
        assert rc == ERR_ARG, (kw, rc)
        msg = lib.cp_last_error()
        assert b"cp_online_realign_activity:" in msg and what.encode() in msg, (kw, msg)

    activity_refused("n_rows", n_rows=0)
    activity_refused("n_rows", n_rows=-1)
    activity_refused("n_rows", n_rows=2 ** 31)
    activity_refused("ldw", ldw=11)
    activity_refused("ldw", ldw=0)
    activity_refused("required", windows=None)
    activity_refused("required", base=None)
    activity_refused("required", gain=None)
    activity_refused("required", activity=None)
    activity_refused("misaligned", windows=addr(w) + 2)
    activity_refused("misaligned", base=addr(base) + 1)
    activity_refused("misaligned", gain=addr(gain) + 2)
    activity_refused("misaligned", activity=addr(act) + 3)

    def refused(what, conf=None, **kw):
        c = _lib.cp_online_realign_config(*[P(**(conf or {}))[k] for k in ("max_lag", "max_lead", "min_len", "min_rest", "context",
                                                                            "min_contrast", "guard")])
        a = dict(dict(activity=act, cue=cue, n_rows=M, segments=seg, n_segments=N, cfg=ctypes.byref(c), expected=exp, table=table,
                      sums=sums), **kw)
        rc = lib.cp_online_realign(a["activity"], a["cue"], a["n_rows"], a["segments"], a["n_segments"], a["cfg"], a["expected"],
                                   a["table"], a["sums"], None)
        assert rc == ERR_ARG, (conf, kw, rc)
        msg = lib.cp_last_error()
        assert b"cp_online_realign:" in msg and what.encode() in msg, (conf, kw, msg)

    refused("n_rows", n_rows=0)
    refused("n_rows", n_rows=-7)
    refused("n_rows", n_rows=2 ** 31)
    refused("n_segments", n_segments=0)
    refused("n_segments", n_segments=65537)
    refused("config", cfg=None)
    refused("max_lag", dict(max_lag=-1))
    refused("max_lag", dict(max_lag=1025))
    refused("max_lead", dict(max_lead=-1))
    refused("max_lead", dict(max_lead=1025))
    refused("context", dict(context=-1))
    refused("context", dict(context=2049))
    refused("min_len", dict(min_len=0))
    refused("min_rest", dict(min_rest=0))
    refused("guard", dict(guard=-1))
    refused("guard", dict(guard=13))
    refused("guard", dict(guard=2 ** 30, min_len=2 ** 31 - 1))
    refused("min_contrast", dict(min_contrast=-1))
    refused("min_contrast", dict(min_contrast=4096))
    for name in ("activity", "cue", "segments", "expected", "table", "sums"):
        refused("required", **{name: None})
    refused("misaligned", activity=addr(act) + 2)
    refused("misaligned", cue=addr(cue) + 1)
    refused("misaligned", segments=addr(seg) + 2)
    refused("misaligned", expected=addr(exp) + 2)
    refused("misaligned", table=addr(table) + 3)
    refused("misaligned", sums=addr(sums) + 4)
