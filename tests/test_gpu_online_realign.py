"""Cue realignment on the MI355X (contrastiveprosthetics_amd/realign.py realign_cues, csrc/online_realign.cuh): the activity
kernel against `activity_reference`, and the expected labels, the segment table and the sums against `realign_reference`.
Every comparison is exact and nothing is excluded."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_online_realign_host import (DEFAULTS, E2E_IDS, E2E_REST, IGNORE, REST, P, cued_recording, lags_nearer_to_the_planted_ones_than_to_zero,
                                      long_region_case, loop_pairs, stepped_recording, tie_case)

pytestmark = pytest.mark.gpu
THREADS = 256                                # the workgroup of or_segment_kernel


def device_realign(activity, cue, segments, p):
    """cp_online_realign on a table of the test's own -> expected, table, sums as `realign_reference` returns them"""
    from contrastiveprosthetics_amd.realign import _realign_dev
    exp, table, sums = _realign_dev(None, np.asarray(activity, dtype=np.int64).clip(-2 ** 31, 2 ** 31 - 1), np.asarray(cue, dtype=np.int32),
                                    np.asarray(segments, dtype=np.int32), p, None, None, torch.device("cuda:0"))
    return exp.astype(np.int64), table, sums


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("expected", "table", "sums")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.nonzero(np.asarray(g != w).reshape(g.shape[0], -1).any(axis=1))[0][:8], g[:4], w[:4])


def same_as_reference(a, cue, segments, p, what=""):
    from contrastiveprosthetics_amd.realign import realign_reference
    want = realign_reference(a, cue, segments, **p)
    got = device_realign(a, cue, segments, p)
    assert_same(got, want, what)
    return want


def n_pairs(row, p):
    s, e, r0, r1 = (int(v) for v in row[:4])
    return len(loop_pairs(np.zeros(r1, dtype=np.int64), s, e, r0, r1, p))


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("ldw", [12, 16])
def test_activity_against_the_reference(ldw):
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.realign import activity_reference
    lib = _lib.load()
    rng = np.random.default_rng(ldw)
    for n in (1, 63, 64, 65, 1000):
        x = (rng.normal(0, 2, (n, 12)) * rng.choice([0.01, 1, 30], (n, 1))).astype(np.float32)
        x = np.where(rng.random((n, 12)) < 0.1, rng.integers(-6, 1200, (n, 12)) * np.float32(0.5), x).astype(np.float32)   # k / 2
        bad = rng.random((n, 12)) < 0.03
        x[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), int(bad.sum()))
        base = rng.normal(0, 0.5, 12).astype(np.float32)
        gain = rng.uniform(0.5, 80, 12).astype(np.float32)
        gain[rng.integers(0, 12, 3)] = 0                                  # channels that add nothing (inf * 0 is NaN: 0)
        if n == 65:
            base, gain = np.zeros(12, dtype=np.float32), np.ones(12, dtype=np.float32)         # the .5 values as they are
        wide = torch.full((n, ldw), float("nan"), device="cuda")
        wide[:, :12] = torch.from_numpy(x).cuda()
        act = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
        rc = lib.cp_online_realign_activity(wide.data_ptr(), ldw, n, base.ctypes.data_as(C.POINTER(C.c_float)),
                                            gain.ctypes.data_as(C.POINTER(C.c_float)), act.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.cp_last_error()
        got = act.cpu().numpy()
        want = activity_reference(x, base, gain)
        assert got[n] == -7 and np.array_equal(got[:n], want), (n, np.nonzero(got[:n] != want)[0][:8])
        assert n < 64 or (want.max() > 0 and np.isnan(x).any() and np.isinf(x).any())


# ---------------------------------------------------------------------------------------------------------------- 2
def test_random_cued_recordings_against_the_reference():
    from contrastiveprosthetics_amd.realign import cue_segments
    rng = np.random.default_rng(8)
    settings = [DEFAULTS, P(max_lag=0), P(max_lead=0), P(context=0, min_rest=1), P(max_lag=1024, max_lead=1024, context=2048),
                P(max_lag=0, max_lead=0, context=0, min_rest=1, min_len=1, guard=0), P(min_contrast=450), P(min_contrast=4095, guard=0, min_len=3)]
    seen = set()
    for trial, p in enumerate(settings):
        M = int(rng.integers(600, 1501))
        a, cue = cued_recording(rng, M, int(rng.integers(1, 13)), noise=int(rng.choice([100, 300])))
        want = same_as_reference(a, cue, cue_segments(cue), p, trial)
        seen |= {(trial, int(st)) for st in want[1][:, 6]}
    assert {st for _, st in seen} >= {0, 1, 2} and (6, 0) in seen and (6, 2) in seen      # min_contrast turns some segments, not all


def test_region_lengths_round_the_scan_s_steps():
    """back-to-back segments are each other's bounds: with a wide context and max_lag a region is its own segment"""
    rng = np.random.default_rng(9)
    lengths = [1, 63, 64, 65, 255, 256, 257, 300]
    edges = np.concatenate([[7], 7 + np.cumsum(lengths)])
    M = int(edges[-1])
    cue = np.full(M, REST)
    a = rng.integers(0, 80, M)
    for i, (s, e) in enumerate(zip(edges[:-1], edges[1:])):
        cue[s:e] = i % 3
        a[s + (e - s) // 3:e - (e - s) // 4] += 900 + 100 * i
    a[5] = 70000                                                         # clamped on load (row 0's region starts at 0)
    a[9] = -3
    p = P(context=2048, max_lag=1024, max_lead=1024, min_len=1, min_rest=1, guard=0)
    segs = np.stack([edges[:-1], edges[1:]], axis=1)
    exp, table, sums = same_as_reference(a, cue, segs, p)
    assert (table[1:, 3] - table[1:, 2]).tolist() == lengths[1:] and table[0, 2:4].tolist() == [0, 8] and (table[1:, 6] == 0).all()
    assert sums[0].sum() == np.clip(a[:8], 0, 4095).sum() != a[:8].sum()
    # the same rows with room on neither side: a region of one window has no pair
    exp, table, sums = same_as_reference(a, cue, segs, P(context=0, max_lag=0, max_lead=1024, min_len=1, min_rest=1, guard=0))
    assert (table[:, 3] - table[:, 2]).tolist() == lengths and table[0, 6] == 1 and (table[1:, 6] == 0).all()
    # L = 4096 is a region, 4097 is not
    M = 4300
    a = rng.integers(0, 60, M)
    a[150:4010] += 3000
    for e, status in ((4000, 0), (4001, 3)):
        cue = np.full(M, REST)
        cue[100:e] = 1
        exp, table, sums = same_as_reference(a, cue, [[100, e]], P(max_lag=96), e)
        assert table[0, 2:4].tolist() == [0, e + 96] and table[0, 6] == status


def test_one_pair_and_one_pair_more_than_the_workgroup_holds():
    from contrastiveprosthetics_amd.realign import cue_segments
    rng = np.random.default_rng(10)
    M = 1000
    cue = np.full(M, REST)
    cue[100:800], cue[800:] = 2, 3                                       # r1 = e: the next segment starts there
    a = rng.integers(0, 50, M)
    a[100:800] += 800
    for p, count in ((P(max_lag=0, max_lead=0), 1), (P(max_lag=0, max_lead=THREADS), THREADS + 1),
                     (P(max_lag=0, max_lead=2 * THREADS), 2 * THREADS + 1), (P(max_lag=3, max_lead=63), THREADS),
                     (P(max_lag=4, max_lead=63), THREADS + 64)):
        exp, table, sums = same_as_reference(a, cue, cue_segments(cue), p, count)
        assert n_pairs(table[0], p) == count and table[0, 6] == 0


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_long_high_region_needs_all_128_bits():
    a, cue, p, want = long_region_case()                                 # (asserts that 64 bits pick another pair)
    got = device_realign(a, cue, [[100, 3900]], p)
    assert_same(got, want, "long region")
    assert got[1][0, 4:7].tolist() == [140, 3930, 0]


# ---------------------------------------------------------------------------------------------------------------- 4
def test_planted_ties_go_where_the_reference_puts_them():
    from contrastiveprosthetics_amd.realign import cue_segments
    a, cue, p = tie_case()
    pairs = loop_pairs(a, 50, 130, 20, 190, p)
    top = max(x[1] for x in pairs if x[0])
    assert sum(1 for x in pairs if x[0] and x[1] == top) > 1              # the data has a tie
    exp, table, sums = same_as_reference(a, cue, cue_segments(cue), p)
    assert table[0, 4:7].tolist() == [72, 92, 0]
    exp, table, sums = same_as_reference(np.full(200, 7), cue, cue_segments(cue), p)           # every pair equal, none has the contrast
    assert table[0, 4:7].tolist() == [50, 70, 2]
    # ties across the waves and the lanes: a flat burst under a long min_len, in a region of several rounds
    M = 1200
    cue = np.full(M, REST)
    cue[200:900] = 5
    a = np.zeros(M, dtype=np.int64)
    a[400:500] = 1000
    p = P(max_lag=300, max_lead=600, min_len=180, min_rest=10, context=150)
    exp, table, sums = same_as_reference(a, cue, cue_segments(cue), p)
    assert table[0, 4:7].tolist() == [320, 500, 0]                        # 80 windows of rest in front: the smallest onset


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_segment_alone_and_among_300_others():
    from contrastiveprosthetics_amd.realign import cue_segments
    rng = np.random.default_rng(12)
    p = P(max_lag=8, max_lead=4, min_len=5, min_rest=2, context=8, guard=2)
    block_cue = np.concatenate([np.full(40, REST), np.full(70, 9), np.full(40, REST)])
    block_a = rng.integers(0, 100, 150)
    block_a[46:113] += 600
    alone = device_realign(block_a, block_cue, cue_segments(block_cue), p)
    assert alone[1][0, 6] == 0
    others_cue, others_a = [], []
    for i in range(300):
        others_cue.append(np.concatenate([np.full(10, i % 7), np.full(int(rng.integers(0, 12)), REST)]))     # some back to back
        act = rng.integers(0, 100, others_cue[-1].shape[0])
        act[int(rng.integers(0, 4)):int(rng.integers(7, 11))] += 500
        others_a.append(act)
    for where in (0, 150, 300):
        cue = np.concatenate(others_cue[:where] + [block_cue] + others_cue[where:])
        a = np.concatenate(others_a[:where] + [block_a] + others_a[where:])
        segs = cue_segments(cue)
        assert segs.shape[0] >= 250
        exp, table, sums = same_as_reference(a, cue, segs, p, where)
        s0 = int(sum(c.shape[0] for c in others_cue[:where])) + 40
        row = int(np.nonzero(segs[:, 0] == s0)[0][0])
        assert row == 0 if where == 0 else row == segs.shape[0] - 1 if where == 300 else 100 < row < segs.shape[0] - 100
        shift = np.array([1, 1, 1, 1, 1, 1, 0, 0]) * (s0 - 40)
        assert np.array_equal(table[row] - shift, alone[1][0]) and np.array_equal(sums[row], alone[2][0])
        r1 = int(table[row, 3])
        assert np.array_equal(exp[s0:r1], alone[0][40:r1 - (s0 - 40)])


# ---------------------------------------------------------------------------------------------------------------- 6
def test_bad_table_rows_get_status_4_and_their_windows_stay():
    """Rows the wrapper would never make, written straight to the device.  A good row takes r0 from the row before and r1 from
    the row behind; where that neighbour is a bad row the definition brings the bound into range (realign.py's docstring), so
    the good rows are compared as well, all of them -- the table is chosen so that their ranges [s, r1) stay apart, which a
    table with bad rows does not promise by itself."""
    from contrastiveprosthetics_amd.realign import realign_reference
    rng = np.random.default_rng(13)
    M = 600
    rows = [[20, 80], [150, 140], [200, 260], [300, 700], [400, 450], [500, 560], [540, 580], [585, 600]]
    bad = [1, 3, 4, 6]                       # s >= e; e > M; starts before its (bad) predecessor's end; before its good one's
    cue = np.full(M, REST)
    a = rng.integers(0, 100, M)
    for i, (s, e) in enumerate(rows):
        cue[max(s, 0):min(e, M)] = i
        a[max(s, 0) + 10:min(e, M)] += 700
    cue[140:150] = 1
    p = P(max_lag=30, max_lead=20, min_len=11, min_rest=3, context=30)
    exp, table, sums = same_as_reference(a, cue, rows, p)
    assert [i for i in range(8) if table[i, 6] == 4] == bad and (table[[0, 2, 5, 7], 6] == 0).all()
    for i in bad:
        assert table[i].tolist() == rows[i] + [-1, -1, -1, -1, 4, -1] and sums[i].tolist() == [0, 0]
    default = np.where(cue < 0, cue, IGNORE)
    for lo, hi in ((140, 150), (300, 400), (450, 500), (560, 585)):      # windows of the bad rows that no good row's range holds
        assert np.array_equal(exp[lo:hi], default[lo:hi])
    # more rows than the cue has windows for, all bad but one
    many = np.array([[5, 40]] + [[3, 2]] * 99)
    exp, table, sums = same_as_reference(a, cue, many, p)
    assert table[0, 6] != 4 and (table[1:, 6] == 4).all()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_two_runs_give_identical_bytes():
    from contrastiveprosthetics_amd.realign import cue_segments
    rng = np.random.default_rng(14)
    a, cue = cued_recording(rng, 1500, 12, noise=300)
    a[:] = np.round(a, -2)                                                # coarse levels: many equal fractions
    runs = [device_realign(a, cue, cue_segments(cue), DEFAULTS) for _ in range(2)]
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 8, 9
@functools.lru_cache(maxsize=1)
def end_to_end():
    from contrastiveprosthetics_amd.online import expected_commands, recording_windows
    raw, labels, planted = stepped_recording()
    raw_d = torch.from_numpy(raw).cuda()
    unit = torch.tensor([[0.0] * 12, [1.0] * 12], device="cuda")
    r = recording_windows(raw_d, unit).cpu().numpy()                      # (r - 0) / 1: the RMS series itself
    mean_std = torch.from_numpy(np.stack([r.mean(0), r.std(0)]).astype(np.float32)).cuda()
    return raw_d, labels, planted, mean_std, expected_commands(labels, E2E_IDS, 0, rest=E2E_REST)


def test_end_to_end_from_a_raw_recording():
    from contrastiveprosthetics_amd import activity_profile, activity_reference, cue_segments, realign_cues, realign_reference, recording_windows
    raw, labels, planted, mean_std, cue = end_to_end()
    w = recording_windows(raw, mean_std)
    out = realign_cues(w, cue)
    host = w.cpu().numpy()
    prof = activity_profile(host, cue)
    exp, table, sums = realign_reference(activity_reference(host, prof["base"], prof["gain"]), cue, cue_segments(cue), **DEFAULTS)
    assert np.array_equal(out["expected"], exp) and out["expected"].dtype == np.int64
    for name, col in (("start", 0), ("end", 1), ("onset", 4), ("offset", 5), ("status", 6), ("cls", 7)):
        assert np.array_equal(out["segments"][name], table[:, col]), name
    assert out["segments"]["status"].tolist() == [0, 0, 0] and out["segments"]["cls"].tolist() == [3, 8, 3]
    assert lags_nearer_to_the_planted_ones_than_to_zero(out["segments"], planted)
    nA = table[:, 5] - table[:, 4]
    assert np.array_equal(out["contrast"], sums[:, 0] / nA - sums[:, 1] / (table[:, 3] - table[:, 2] - nA))
    # with the profile given, and on a strided view of wider rows
    wide = torch.zeros(w.shape[0], 16, device="cuda")
    wide[:, :12] = w
    again = realign_cues(wide[:, :12], cue, prof)
    assert np.array_equal(again["expected"], exp)


def test_enroll_takes_the_realigned_labels_and_counts_their_windows():
    from contrastiveprosthetics_amd import OnlineDecoder, realign_cues, recording_windows, sample_labels
    from contrastiveprosthetics_amd.engine import Engine
    raw, labels, planted, mean_std, cue = end_to_end()
    e = Engine(adabn=False, dtype="f32", device="cuda:0", seed=3)
    e.init_parameters(3)
    dec = OnlineDecoder(e, mean_std[0], mean_std[1], classes=E2E_IDS + [20])
    out = realign_cues(recording_windows(raw, dec.mean_std), cue)
    counts = dec.enroll(raw, sample_labels(out["expected"], raw.shape[0]))
    want = {c: int((out["expected"] == c).sum()) for c in E2E_IDS + [20]}
    assert counts == want and want[20] == 0 and min(want[3], want[8]) > 50
    assert sum(want.values()) < int((cue >= 0).sum())                     # fewer than the cue labelled: the lags and guards are out
