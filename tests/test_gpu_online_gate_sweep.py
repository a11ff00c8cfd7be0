"""The gate sweep on the MI355X (contrastiveprosthetics_amd/online.py sweep_gate, csrc/online_gate.cuh og_rows_kernel and
og_sweep_kernel) against the numpy restatement of the gate (tests/test_online_gate_host.py GateReference) followed by
`score_commands`, and against the shipped gate on the device.  Every comparison is exact and nothing is excluded."""
import functools

import numpy as np
import pytest
import torch

from test_online_gate_host import GateReference

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("n_cue", "n_rest", "hit", "wrong", "false_active", "switches", "segments", "reached", "latency_sum", "wrong_segments")
M, G = 600, 200
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# a cued recording's logits, random configs and the oracle (host only)
# ---------------------------------------------------------------------------------------------------------------------------
def recording(K, m=M, seed=0):
    """ids (K,), logits (m, K) f32 and expected (m,): rest stretches, then cue segments of 30..80 windows in which the cued class
    is raised by a margin that ramps up over the first 12 windows; two windows between them are not scored (the cue changes
    inside them).  The noise is as wide as the raise, so the runner-up sometimes wins and rest sometimes passes a threshold."""
    from contrastiveprosthetics_amd.online import IGNORE, REST
    rng = np.random.default_rng(1000 * K + seed)
    ids = np.sort(rng.choice(200, K, replace=False)).astype(np.int64)
    lg = rng.uniform(-0.25, 0.35, (m, K))
    exp = np.full(m, IGNORE, dtype=np.int64)
    j = int(rng.integers(3, 10))
    exp[:j] = REST
    while j < m:
        c, n = int(rng.integers(K)), int(rng.integers(30, 81))
        t = np.arange(min(n, m - j))
        lg[j:j + n, c] += 0.45 * np.minimum(1.0, (t + 1) / 12.0)
        exp[j:j + n] = ids[c]
        j += n + 2
        r = int(rng.integers(0, 40))                       # (0: the next cue follows after the two unscored windows)
        exp[j:j + r] = REST
        j += r + (2 if r else 0)
    return ids, lg.astype(F), exp


def random_configs(ids, n=G, seed=0):
    """n config dicts over the whole range of the settings: vote 1..256 (small rings more often, the ends and the 64-row block
    size always), min_votes 1..vote+1 (vote+1: never a candidate), dwell 1..12, release 0..12, both weights, min_margin 0..0.3,
    per-class thresholds (now and then one float for all)."""
    rng = np.random.default_rng(77 + seed)
    out = []
    for g in range(n):
        vote = [1, 256, 64, 65, 63, 255, 2, 128][g] if g < 8 else \
            int(rng.integers(*[(1, 17), (17, 65), (65, 257)][int(rng.choice(3, p=[0.5, 0.35, 0.15]))]))
        thr = {int(i): float(F(rng.uniform(0.05, 0.6))) for i in ids}
        cfg = dict(vote=vote, min_votes=int(rng.integers(1, vote + 2)) if rng.random() < 0.5 else int(rng.integers(1, 4)),
                   dwell=int(rng.integers(1, 13)), release=int(rng.integers(0, 13)), weight=["count", "margin"][int(rng.integers(2))],
                   min_margin=float(F(rng.uniform(0.0, 0.3))), min_cosine=thr if rng.random() < 0.8 else float(F(rng.uniform(0.0, 0.5))))
        if rng.random() < 0.3:
            cfg["min_votes"] = min(cfg["min_votes"], vote)
        out.append(cfg)
    return out


def oracle(ids, lg, exp, cfg):
    """GateReference from its zero state over the rows, then score_commands -> (commands (m,) int32 class ids, scores dict)"""
    from contrastiveprosthetics_amd.online import score_commands
    mc = cfg.get("min_cosine", -2.0)
    thr = np.array([mc.get(int(i), cfg.get("default", -2.0)) for i in ids], dtype=F) if isinstance(mc, dict) else F(mc)
    ref = GateReference(ids, thr, cfg.get("vote", 25), cfg.get("min_votes", 1), cfg.get("dwell", 1), cfg.get("release", 1),
                        cfg.get("weight", "count"), cfg.get("min_margin", 0.0))
    cmd = ref.run_rows(lg)[0]
    return cmd, score_commands(cmd, exp)


@functools.lru_cache(maxsize=None)
def case(K):
    """the recording of K classes, its G configs and the oracle's answer for each of them, computed once and left unchanged"""
    ids, lg, exp = recording(K)
    configs = random_configs(ids)
    want = [oracle(ids, lg, exp, c) for c in configs]
    cmds = np.stack([w[0] for w in want])
    scores = {k: np.array([w[1][k] for w in want], dtype=np.int64) for k in KEYS}
    for a in (ids, lg, exp, cmds, *scores.values()):
        a.setflags(write=False)
    return ids, lg, exp, configs, cmds, scores


def assert_data_makes_the_score_work(scores, never=()):
    """from the oracle alone: the counters a setting moves are non-zero for some config and differ between two"""
    for k in ("hit", "wrong", "false_active", "switches", "latency_sum"):
        if k not in never:
            assert scores[k].max() > 0 and np.unique(scores[k]).size >= 2, (k, scores[k])


def sweep(lg_dev, exp, ids, configs):
    from contrastiveprosthetics_amd.online import sweep_gate
    scores, cmds = sweep_gate(lg_dev, exp, ids, configs, return_commands=True)
    assert tuple(scores) == KEYS and cmds.dtype == torch.int32 and cmds.shape == (len(configs), lg_dev.shape[0])
    return scores, cmds.cpu().numpy()


def assert_equal(got_scores, got_cmds, want_scores, want_cmds, what):
    for k in KEYS:
        bad = np.nonzero(got_scores[k] != want_scores[k])[0]
        assert bad.size == 0, (what, k, bad[:5], got_scores[k][bad[:5]], want_scores[k][bad[:5]])
    bad = np.argwhere(got_cmds != want_cmds)
    assert bad.shape[0] == 0, (what, "commands", bad[:5])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. counters and commands against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,ldl", [(1, 1), (5, 5), (64, 64), (5, 64)])
def test_counters_and_commands_against_the_oracle(K, ldl):
    ids, lg, exp, configs, want_cmds, want = case(K)
    # one class is never wrong (there is no other grasp to take)
    assert_data_makes_the_score_work(want, never=("wrong",) if K == 1 else ())
    assert any(c["min_votes"] == c["vote"] + 1 for c in configs) and {c["weight"] for c in configs} == {"count", "margin"}
    dev = torch.zeros(M, ldl, device="cuda")
    dev[:, :K] = torch.from_numpy(lg)
    view = dev[:, :K]                                                  # K < ldl: the rows as a multi-stream push packs them
    assert view.stride(0) == ldl
    scores, cmds = sweep(view, exp, ids, configs)
    assert_equal(scores, cmds, want, want_cmds, (K, ldl))
    from contrastiveprosthetics_amd.online import sweep_gate
    alone = sweep_gate(view, exp, ids, configs)                        # without the commands: the same table
    assert all(np.array_equal(alone[k], want[k]) for k in KEYS)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the shipped gate on the device
# ---------------------------------------------------------------------------------------------------------------------------
class Ids:
    """the part of a single-stream decoder that CommandGate.apply reads"""
    device = torch.device("cuda:0")
    phase, n_seen = 0, 0

    def __init__(self, ids, vote):
        self.class_ids, self.vote = torch.as_tensor(ids, dtype=torch.int32), vote

    def push(self, *a, **k):
        raise AssertionError("apply() does not push the decoder")


@pytest.mark.parametrize("K", [5, 64])
def test_commands_equal_the_shipped_gate_in_any_cut(K):
    from contrastiveprosthetics_amd.online import CommandGate
    ids, lg, exp, configs, _, _ = case(K)
    pick = [0, 1, 2, 3, 11, 57, 120, 199]                              # votes 1, 256, 64, 65 and four random ones
    dev = torch.from_numpy(lg).cuda()
    _, cmds = sweep(dev, exp, ids, [configs[g] for g in pick])
    assert len({tuple(c) for c in cmds.tolist()}) >= 4                 # (not eight times the same sequence)
    for row, g in zip(cmds, pick):
        for cut in (M, 1, 16, 256):
            gate = CommandGate(Ids(ids, 25), vote=configs[g]["vote"])
            gate.use(configs[g])
            got = torch.cat([gate.apply(dev[p:p + cut])[0] for p in range(0, M, cut)]).cpu().numpy()
            assert np.array_equal(got, row), (K, g, cut)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. block edges: the 64-row load, the ring wrap and the tail block
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 128, 257])
def test_block_edges(m):
    ids, lg, exp, _, _, _ = case(5)
    lg, exp = lg[:m], exp[:m]
    thr = {int(i): 0.3 for i in ids}
    configs = [dict(vote=v, min_cosine=thr, **kw) for v in (1, 64, 256)
               for kw in (dict(), dict(weight="margin", dwell=2, release=3, min_margin=0.05), dict(min_votes=min(v, 3), dwell=3, release=0))]
    want = [oracle(ids, lg, exp, c) for c in configs]
    scores, cmds = sweep(torch.from_numpy(lg).cuda(), exp, ids, configs)
    assert_equal(scores, cmds, {k: np.array([w[1][k] for w in want]) for k in KEYS}, np.stack([w[0] for w in want]), m)
    if m >= 63:
        assert (cmds >= 0).any() and len({tuple(c) for c in cmds.tolist()}) >= 3


# ---------------------------------------------------------------------------------------------------------------------------
# 4. independence of the configs in one call
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_config_does_not_depend_on_its_neighbours():
    ids, lg, exp, configs, want_cmds, want = case(5)
    t = 17
    assert want["hit"][t] > 0 and want["switches"][t] > 2
    others = (configs[:t] + configs[t + 1:]) * 2                       # 398 other configs
    dev = torch.from_numpy(lg).cuda()
    # alone; first, last and in the middle of 300 (75 full workgroups); last of 299 and of 301 (a part-filled last workgroup)
    places = {"alone": ([configs[t]], 0), "first": ([configs[t]] + others[:299], 0), "last": (others[:299] + [configs[t]], 299),
              "middle": (others[:150] + [configs[t]] + others[150:299], 150), "last of 299": (others[:298] + [configs[t]], 298),
              "last of 301": (others[:300] + [configs[t]], 300)}
    for name, (cfgs, at) in places.items():
        scores, cmds = sweep(dev, exp, ids, cfgs)
        assert np.array_equal(cmds[at], want_cmds[t]), name
        assert all(scores[k][at] == want[k][t] for k in KEYS), name
        if name == "last of 301":                                      # and the neighbours are themselves
            assert np.array_equal(cmds[:t], want_cmds[:t]) and np.array_equal(scores["hit"][:t], want["hit"][:t])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. non-finite rows
# ---------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_are_rejected_as_the_gate_rejects_them():
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
    scores, cmds = sweep(torch.from_numpy(lg).cuda(), exp, ids, configs)
    assert_equal(scores, cmds, {k: np.array([w[1][k] for w in want]) for k in KEYS}, np.stack([w[0] for w in want]), "non-finite")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. every gate open: the command is the decoder's vote
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=False, dtype="f32", device="cuda:0", seed=3)
    e.init_parameters(3)
    g = torch.Generator().manual_seed(3)
    labels = torch.arange(41).repeat(4).cuda()
    for _ in range(3):
        x = (torch.randn(4 * 41, 12, generator=g) * 1.5 + 0.3).cuda()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(PARAMS)
    torch.cuda.synchronize()
    return e


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_gate_open_command_is_the_decoders_vote(engine, dtype):
    from contrastiveprosthetics_amd.online import IGNORE, OnlineDecoder, sweep_gate
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rng = np.random.default_rng(21)
    rec = torch.from_numpy((rng.standard_normal((6000, 12)) * 2e-3).astype(F)).cuda()
    w = preprocess_segments(rec[None, :3000], keep=20 * np.arange(140))[0]
    dec = OnlineDecoder(engine, w.mean(0), w.std(0), classes=[30, 2, 17, 5, 9, 40, 0], dtype=dtype)
    pred, voted, logits = dec.push(rec, return_logits=True)
    m = logits.shape[0]
    assert m == 300
    scores, cmds = sweep_gate(logits, np.full(m, IGNORE), dec.class_ids, [{}], return_commands=True)
    assert torch.equal(cmds[0], voted)
    assert scores["switches"][0] == int((voted[1:] != voted[:-1]).sum()) + 1 and scores["n_cue"][0] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 7. config values the wrapper would refuse, written straight to the device array
# ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_config_values_score_minus_one_and_touch_nothing():
    """a validity check of the kernel's early return: such a config must not index anything"""
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import _sweep_configs
    ids, lg, exp, configs, want_cmds, want = case(5)
    lib = _lib.load()
    n = 7                                                              # two workgroups, the second part-filled
    cfg, thr = _sweep_configs(configs[:n], ids)
    bad = {1: (0, 0), 3: (0, 257), 4: (2, 0), 5: (1, 0), 6: (3, -1)}   # config: (field, value): vote, dwell, min_votes, release
    for g, (field, value) in bad.items():
        cfg[g, field] = value
    slot = {int(c): k for k, c in enumerate(ids)}
    exp_d = torch.tensor([slot.get(int(e), int(e)) for e in exp], dtype=torch.int32, device="cuda")
    dev, cfg_d, thr_d = torch.from_numpy(lg).cuda(), torch.from_numpy(cfg).cuda(), torch.from_numpy(thr).cuda()
    scratch = torch.empty(lib.cp_online_gate_sweep_scratch_bytes(M), dtype=torch.uint8, device="cuda")
    scores = torch.full((n, 10), -99, dtype=torch.int64, device="cuda")
    cmds = torch.full((n, M), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.cp_online_gate_sweep(dev.data_ptr(), 5, M, 5, exp_d.data_ptr(), cfg_d.data_ptr(), thr_d.data_ptr(), n,
                                        scratch.data_ptr(), scratch.numel(), scores.data_ptr(), cmds.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "cp_online_gate_sweep")
    scores, cmds = scores.cpu().numpy(), cmds.cpu().numpy()
    for g in range(n):
        if g in bad:
            assert (scores[g] == -1).all() and (cmds[g] == -7).all(), g
        else:                                                          # slots here, class ids in the oracle
            assert scores[g].tolist() == [want[k][g] for k in KEYS], g
            assert np.array_equal(np.where(cmds[g] >= 0, ids[np.maximum(cmds[g], 0)], -1), want_cmds[g]), g
