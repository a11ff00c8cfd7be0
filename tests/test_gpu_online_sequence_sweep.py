"""The sequence sweep on the MI355X (contrastiveprosthetics_amd/sequence.py sweep_sequence, csrc/online_sequence.cuh
seq_rows_kernel and seq_sweep_kernel) against the numpy definition (sequence.SequenceReference) followed by `score_commands`,
and against the shipped stage on the device.  Every comparison is exact and nothing is excluded."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_online_gate_sweep import KEYS, assert_data_makes_the_score_work, assert_equal, recording
from test_gpu_online_sequence import Ids

pytestmark = pytest.mark.gpu

F = np.float32
M, G = 600, 200


def models(K):
    """8 cost matrices: potts with and without the way through rest, from the cues, dense, and none at all"""
    from contrastiveprosthetics_amd.sequence import potts, transitions_from_cues
    ids, _, exp = recording(K)
    rng = np.random.default_rng(K)
    dense = rng.integers(0, 1 << 20, (K + 1, K + 1)).astype(np.int32)
    dense[rng.integers(0, K + 1), rng.integers(0, K + 1)] = 1 << 28
    return [dict(switch=0.5, engage=0.5, release=0.5), dict(switch=0.25, engage=0.125, release=0.375, through_rest=True),
            potts(K, 1.0, 0.75, 0.0625), transitions_from_cues(exp, ids, 0.125), transitions_from_cues(exp, ids, 0.5, floor_count=0),
            dense, np.zeros((K + 1, K + 1), dtype=np.int32), lambda i: potts(len(i), 0.03125, 2.0, 300.0)]


def random_configs(K, n=G, seed=0):
    """n config dicts: one of 8 models, lag over 0..63 with both ends (and 1, 62) always there, per-class thresholds (now and
    then one float for all, or none)"""
    ids = recording(K)[0]
    rng = np.random.default_rng(99 + seed)
    mods = models(K)
    out = []
    for g in range(n):
        cfg = dict(transitions=mods[g % 8 if g < 16 else int(rng.integers(8))],
                   lag=[0, 63, 1, 62][g] if g < 4 else int(rng.integers(0, 64)))
        u = rng.random()
        if u < 0.7:
            cfg["min_cosine"] = {int(i): float(F(rng.uniform(0.0, 0.5))) for i in ids}
        elif u < 0.9:
            cfg["min_cosine"] = float(F(rng.uniform(0.0, 0.4)))
        out.append(cfg)
    return out


def oracle(ids, lg, exp, cfg):
    """SequenceReference from its zero state over the rows, then score_commands -> (commands (m,) int32 class ids, scores dict)"""
    from contrastiveprosthetics_amd.online import score_commands
    from contrastiveprosthetics_amd.sequence import SequenceReference, _matrix_for
    mc = cfg.get("min_cosine", -2.0)
    thr = np.array([mc.get(int(i), cfg.get("default", -2.0)) for i in ids], dtype=F) if isinstance(mc, dict) else F(mc)
    t = cfg.get("transitions", dict(switch=0.5, engage=0.5, release=0.5))
    cmd = SequenceReference(ids, thr, _matrix_for(t, np.asarray(ids)), cfg.get("lag", 0)).run_rows(lg)[0]
    return cmd, score_commands(cmd, exp)


@functools.lru_cache(maxsize=None)
def case(K):
    """the recording of K classes, its G configs and the oracle's answer for each of them, computed once and left unchanged"""
    ids, lg, exp = recording(K)
    configs = random_configs(K)
    want = [oracle(ids, lg, exp, c) for c in configs]
    cmds = np.stack([w[0] for w in want])
    scores = {k: np.array([w[1][k] for w in want], dtype=np.int64) for k in KEYS}
    for a in (ids, lg, exp, cmds, *scores.values()):
        a.setflags(write=False)
    return ids, lg, exp, configs, cmds, scores


def sweep(lg_dev, exp, ids, configs):
    from contrastiveprosthetics_amd.sequence import sweep_sequence
    scores, cmds = sweep_sequence(lg_dev, exp, ids, configs, return_commands=True)
    assert tuple(scores) == KEYS and cmds.dtype == torch.int32 and cmds.shape == (len(configs), lg_dev.shape[0])
    return scores, cmds.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. counters and commands against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,ldl", [(1, 1), (5, 5), (64, 64), (5, 64)])
def test_counters_and_commands_against_the_oracle(K, ldl):
    from contrastiveprosthetics_amd.sequence import _sweep_configs, sweep_sequence
    ids, lg, exp, configs, want_cmds, want = case(K)
    # one class is never wrong (there is no other grasp to take)
    assert_data_makes_the_score_work(want, never=("wrong",) if K == 1 else ())
    assert {c["lag"] for c in configs} >= {0, 1, 62, 63} and _sweep_configs(configs, ids)[0].shape[0] == 8
    dev = torch.zeros(M, ldl, device="cuda")
    dev[:, :K] = torch.tensor(lg)
    view = dev[:, :K]                                                  # K < ldl: the rows as a multi-stream push packs them
    assert view.stride(0) == ldl
    scores, cmds = sweep(view, exp, ids, configs)
    assert_equal(scores, cmds, want, want_cmds, (K, ldl))
    alone = sweep_sequence(view, exp, ids, configs)                    # without the commands: the same table
    assert all(np.array_equal(alone[k], want[k]) for k in KEYS)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the shipped stage on the device
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 64])
def test_commands_equal_a_fresh_stage_on_the_device(K):
    from contrastiveprosthetics_amd.sequence import SequenceGate
    ids, lg, exp, configs, _, _ = case(K)
    pick = [0, 1, 2, 3, 5, 11, 57, 120, 199]                           # lags 0, 63, 1, 62 and five other configs
    dev = torch.tensor(lg).cuda()
    _, cmds = sweep(dev, exp, ids, [configs[g] for g in pick])
    assert len({tuple(c) for c in cmds.tolist()}) >= 5                 # (not nine times the same sequence)
    for row, g in zip(cmds, pick):
        for cut in (M, 256, 16):
            gate = SequenceGate(Ids(ids))
            gate.use(configs[g])
            got = torch.cat([gate.apply(dev[p:p + cut])[0] for p in range(0, M, cut)]).cpu().numpy()
            assert np.array_equal(got, row), (K, g, cut)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. block edges: the 64-row block, the ring wrap and the tail block
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 128, 257])
def test_block_edges(m):
    ids, lg, exp, _, _, _ = case(5)
    lg, exp = lg[:m], exp[:m]
    configs = [dict(lag=lag, min_cosine=0.25, transitions=t) for lag in (0, 1, 63) for t in models(5)[:3]]
    want = [oracle(ids, lg, exp, c) for c in configs]
    scores, cmds = sweep(torch.tensor(lg).cuda(), exp, ids, configs)
    assert_equal(scores, cmds, {k: np.array([w[1][k] for w in want]) for k in KEYS}, np.stack([w[0] for w in want]), m)
    if m >= 63:
        assert (cmds >= 0).any() and len({tuple(c) for c in cmds.tolist()}) >= 3


# ---------------------------------------------------------------------------------------------------------------------------
# 4. independence of the configs in one call
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_config_does_not_depend_on_its_neighbours():
    ids, lg, exp, configs, want_cmds, want = case(5)
    dev = torch.tensor(lg).cuda()
    scores, cmds = sweep(dev, exp, ids, configs[::-1])                 # the reversed order: every config at another place
    assert_equal({k: v[::-1] for k, v in scores.items()}, cmds[::-1], want, want_cmds, "reversed")
    t = 17
    assert want["hit"][t] > 0 and want["switches"][t] > 2
    others = configs[:t] + configs[t + 1:]
    # alone; first, last and in the middle of 100 (25 full workgroups); last of 99 and of 101 (a part-filled last workgroup)
    places = {"alone": ([configs[t]], 0), "first": ([configs[t]] + others[:99], 0), "last": (others[:99] + [configs[t]], 99),
              "middle": (others[:50] + [configs[t]] + others[50:99], 50), "last of 99": (others[:98] + [configs[t]], 98),
              "last of 101": (others[:100] + [configs[t]], 100)}
    for name, (cfgs, at) in places.items():
        scores, cmds = sweep(dev, exp, ids, cfgs)
        assert np.array_equal(cmds[at], want_cmds[t]), name
        assert all(scores[k][at] == want[k][t] for k in KEYS), name


# ---------------------------------------------------------------------------------------------------------------------------
# 5. non-finite rows
# ---------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_carry_no_evidence():
    ids, lg, exp, configs, _, _ = case(5)
    m = 300
    lg, exp = lg[:m].copy(), exp[:m]
    rng = np.random.default_rng(9)
    rows = rng.choice(m, 24, replace=False)
    lg[rows[:12], rng.integers(0, 5, 12)] = np.nan
    lg[rows[12:20], rng.integers(0, 5, 8)] = np.inf
    lg[rows[20:]] = np.inf                                             # whole rows
    configs = configs[:24]
    want = [oracle(ids, lg, exp, c) for c in configs]
    clean = case(5)[4][:24, :m]
    assert sum(not np.array_equal(w[0], c) for w, c in zip(want, clean)) >= 5      # the rows matter to the commands
    scores, cmds = sweep(torch.tensor(lg).cuda(), exp, ids, configs)
    assert_equal(scores, cmds, {k: np.array([w[1][k] for w in want]) for k in KEYS}, np.stack([w[0] for w in want]), "non-finite")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. pick_gate picks from the table unchanged
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 64])
def test_pick_gate_returns_the_index_the_oracle_gives(K):
    from contrastiveprosthetics_amd.online import pick_gate
    from contrastiveprosthetics_amd.sequence import sweep_sequence
    ids, lg, exp, configs, _, want = case(K)
    scores = sweep_sequence(torch.tensor(lg).cuda(), exp, ids, configs)
    for limits in (dict(), dict(max_false_rate=0.2, max_wrong_rate=0.02), dict(max_false_rate=0.0, max_wrong_rate=0.0)):
        assert pick_gate(scores, **limits) == pick_gate(want, **limits), limits
    assert pick_gate(want, max_false_rate=0.2, max_wrong_rate=0.02) is not None


# ---------------------------------------------------------------------------------------------------------------------------
# 7. config values the wrapper would refuse, written straight to the device array
# ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_config_values_score_minus_one_and_touch_nothing():
    """a validity check of the kernel's early return: such a config must not index anything"""
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.sequence import _sweep_configs
    ids, lg, exp, configs, want_cmds, want = case(5)
    lib = _lib.load()
    n = 7                                                              # two workgroups, the second part-filled
    costs, cfg, thr = _sweep_configs(configs[:n], ids)
    n_models = costs.shape[0]
    bad = {1: (1, -1), 3: (1, 64), 4: (0, -1), 5: (0, n_models), 6: (1, 1 << 30)}      # config: (field, value): model, lag
    for g, (field, value) in bad.items():
        cfg[g, field] = value
    slot = {int(c): k for k, c in enumerate(ids)}
    exp_d = torch.tensor([slot.get(int(e), int(e)) for e in exp], dtype=torch.int32, device="cuda")
    dev, cfg_d, thr_d, costs_d = (torch.tensor(x).cuda() for x in (lg, cfg, thr, costs))
    scratch = torch.empty(lib.cp_online_seq_sweep_scratch_bytes(M), dtype=torch.uint8, device="cuda")
    scores = torch.full((n, 10), -99, dtype=torch.int64, device="cuda")
    cmds = torch.full((n, M), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.cp_online_seq_sweep(dev.data_ptr(), 5, M, 5, exp_d.data_ptr(), costs_d.data_ptr(), n_models, cfg_d.data_ptr(),
                                       thr_d.data_ptr(), n, scratch.data_ptr(), scratch.numel(), scores.data_ptr(), cmds.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "cp_online_seq_sweep")
    scores, cmds = scores.cpu().numpy(), cmds.cpu().numpy()
    for g in range(n):
        if g in bad:
            assert (scores[g] == -1).all() and (cmds[g] == -7).all(), g
        else:                                                          # slots here, class ids in the oracle
            assert scores[g].tolist() == [want[k][g] for k in KEYS], g
            assert np.array_equal(np.where(cmds[g] >= 0, ids[np.maximum(cmds[g], 0)], -1), want_cmds[g]), g
