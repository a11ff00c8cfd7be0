"""The grasp sequence decoder on the MI355X (contrastiveprosthetics_amd/sequence.py SequenceGate, csrc/online_sequence.cuh
seq_push_kernel) against its numpy definition (sequence.SequenceReference) and behind the decoders.  Every comparison is exact
and nothing is excluded."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_online_gate_sweep import PARAMS, recording
from test_online_sequence_host import floor_rows

pytestmark = pytest.mark.gpu

F = np.float32
M = 600
LAGS = (0, 1, 25, 63)


class Ids:
    """the part of a decoder that SequenceGate.apply reads"""
    device = torch.device("cuda:0")
    phase = 0

    def __init__(self, ids, multi=False):
        cid = [None if i is None else torch.as_tensor(np.array(i), dtype=torch.int32) for i in (ids if multi else [ids])]
        self.class_ids = cid if multi else cid[0]
        self.n_seen = np.zeros(len(cid), dtype=np.int64) if multi else 0

    def push(self, *a, **k):
        raise AssertionError("apply() does not push the decoder")


def matrix(kind, K):
    from contrastiveprosthetics_amd.sequence import potts
    if kind == "potts":
        return potts(K, 0.5, 0.5, 0.5)
    if kind == "through_rest":
        return potts(K, 0.5, 0.25, 0.125, through_rest=True)
    rng = np.random.default_rng(K)
    c = rng.integers(0, 1 << 20, (K + 1, K + 1)).astype(np.int32)      # dense: up to one cosine unit, the diagonal not zero
    c[rng.integers(0, K + 1), rng.integers(0, K + 1)] = 1 << 28
    return c


@functools.lru_cache(maxsize=None)
def want(K, kind, lag, thr=0.25):
    """the definition over recording(K), computed once and left unchanged: (command, now, lead), score, ring"""
    from contrastiveprosthetics_amd.sequence import SequenceReference
    ids, lg, _ = recording(K)
    ref = SequenceReference(ids, thr, matrix(kind, K), lag)
    out = ref.run_rows(lg)
    for a in (*out, ref.score, *ref.ring):
        a.setflags(write=False)
    return out, ref.score, ref.ring, ref.n


def run_cuts(gate, dev, cuts):
    outs, p = [], 0
    for n in cuts:
        outs.append(gate.apply(dev[p:p + n]))
        p += n
    assert p == dev.shape[0]
    return [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(3)]


def assert_same(got, wanted, what):
    for name, g, w in zip(("command", "now", "lead"), got, wanted):
        bad = np.nonzero(g != w)[0]
        assert g.dtype == np.int32 and bad.size == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


def assert_state(gate, score, ring, n, what, stream=0):
    st = gate.state(stream)
    assert st["n"] == n and np.array_equal(st["score"], score), (what, st["n"], st["score"], score)
    assert len(st["ring"]) == len(ring) and all(np.array_equal(a, b) for a, b in zip(st["ring"], ring)), what


# ---------------------------------------------------------------------------------------------------------------------------
# 1. outputs and state against the definition, in any cut
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["potts", "through_rest", "dense"])
@pytest.mark.parametrize("K", [1, 2, 41, 64])
def test_outputs_and_state_equal_the_definition_in_any_cut(K, kind):
    from contrastiveprosthetics_amd.sequence import SequenceGate
    ids, lg, _ = recording(K)
    dev = torch.from_numpy(lg).cuda()
    rng = np.random.default_rng(K)
    pieces = []
    while sum(pieces) < M:
        pieces.append(int(min(rng.integers(1, 300), M - sum(pieces))))
    C = matrix(kind, K)
    seen = set()
    for lag in LAGS:
        out, score, ring, n = want(K, kind, lag)
        seen.update(out[0].tolist())
        assert (out[0][:lag] == -1).all()
        for cuts in ([M], [1] * M, [16] * 37 + [8], [256, 256, 88], pieces):
            gate = SequenceGate(Ids(ids), transitions=lambda i: C, min_cosine=0.25, lag=lag)
            assert_same(run_cuts(gate, dev, cuts), out, (K, kind, lag, cuts[:3]))
            assert_state(gate, score, ring, n, (K, kind, lag, cuts[:3]))
    assert -1 in seen and len(seen) >= min(K, 3) + 1                   # none and grasps are commanded


def test_the_data_makes_the_test_work():
    """from the definition alone, K = 41, potts 0.5, min_cosine 0.25, lag 0: far fewer switches than raw argmax and fewer wrong"""
    from contrastiveprosthetics_amd.online import score_commands
    ids, lg, exp = recording(41)
    raw = score_commands(ids[lg.argmax(axis=1)], exp)
    dec = score_commands(want(41, "potts", 0)[0][0], exp)
    print("raw argmax", raw, "decoder", dec)
    assert dec["switches"] * 4 < raw["switches"] and dec["wrong"] < raw["wrong"]
    assert (raw["switches"], raw["wrong"]) == (369, 131) and (dec["switches"], dec["wrong"]) == (33, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. 256 streams in one launch; a stream without a model
# ---------------------------------------------------------------------------------------------------------------------------
def test_256_streams_in_one_launch_each_equal_their_own_stage():
    from contrastiveprosthetics_amd.sequence import SequenceGate, SequenceReference, potts
    rng = np.random.default_rng(5)
    S, launches = 256, 10
    ks = rng.choice([1, 2, 3, 5, 17, 41, 64], S)
    lags = rng.choice([0, 1, 2, 7, 25, 63], S).tolist()
    ids = [np.sort(rng.choice(300, k, replace=False)) for k in ks]
    thr = [(rng.integers(0, 24, k) / 64.0).astype(F) for k in ks]

    def trans(i):                                                      # one matrix per K: dense for odd K
        return matrix("dense", len(i)) if len(i) % 2 else potts(len(i), 0.375, 0.5, 0.25)

    many = SequenceGate(Ids(ids, multi=True), transitions=trans, lag=lags)
    for s in range(S):
        many.set_thresholds(s, {int(i): float(t) for i, t in zip(ids[s], thr[s])})
    m = rng.integers(0, 13, (launches, S)) * (rng.random((launches, S)) > 0.25)        # some streams sit a launch out
    m[:, 7] = 0                                                                       # and one never has a row
    total = m.sum(axis=0)
    lgs = [rng.uniform(-0.25, 0.6, (int(total[s]), int(ks[s]))).astype(F) for s in range(S)]
    dev = [torch.from_numpy(x).cuda() for x in lgs]
    pos = np.zeros(S, dtype=np.int64)
    got = [[] for _ in range(S)]
    for r in range(launches):
        packed = torch.full((int(m[r].sum()), 64), float("nan"), device="cuda")     # as a multi-stream push packs them:
        row0 = np.concatenate([[0], np.cumsum(m[r])[:-1]])                           # columns past K_s are never read
        views = []
        for s in range(S):
            if m[r, s] == 0:
                views.append(None if s % 2 else dev[s][:0])
                continue
            v = packed[row0[s]:row0[s] + m[r, s], :ks[s]]
            v.copy_(dev[s][pos[s]:pos[s] + m[r, s]])
            views.append(v)
        out = many.apply(views)
        for s in range(S):
            got[s].append(out[s])
        pos += m[r]
    for s in range(S):
        g = [torch.cat([o[i] for o in got[s]]).cpu().numpy() for i in range(3)]
        ref = SequenceReference(ids[s], thr[s], trans(ids[s]), lags[s])
        assert_same(g, ref.run_rows(lgs[s]), ("definition", s, int(ks[s]), lags[s]))
        assert_state(many, ref.score, ref.ring, ref.n, s, stream=s)
        if total[s]:
            own = SequenceGate(Ids(ids[s]), transitions=trans, min_cosine={int(i): float(t) for i, t in zip(ids[s], thr[s])},
                               lag=lags[s])
            assert_same(g, run_cuts(own, dev[s], [int(total[s])]), ("own stage", s))
            assert_state(own, ref.score, ref.ring, ref.n, s)
    assert many.state(7)["n"] == 0 and many.state(7)["ring"] == []


def test_a_stream_without_a_model_is_left_unwritten():
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.sequence import SequenceGate, SequenceReference, potts
    ids = np.array([3, 8, 9])
    lg = np.random.default_rng(2).uniform(-0.2, 0.6, (30, 3)).astype(F)
    gate = SequenceGate(Ids([ids, None, ids], multi=True), lag=[0, 0, 2])
    gate.apply([torch.from_numpy(lg[:0]).cuda(), None, None])         # installs the models of streams 0 and 2
    lib = _lib.load()
    dev = torch.from_numpy(lg).cuda()
    rm = torch.tensor([[0, 10, 20], [10, 10, 10]], dtype=torch.int32, device="cuda")
    out = torch.full((3, 30), -7, dtype=torch.int32, device="cuda")
    before = gate.ws.clone()
    _lib.check(lib.cp_online_seq_push(3, gate.ws.data_ptr(), gate.ws.numel(), dev.data_ptr(), 3, rm[0].data_ptr(), rm[1].data_ptr(), 30,
                                      out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "cp_online_seq_push")
    out = out.cpu().numpy()
    assert (out[:, 10:20] == -7).all()
    per = 4 * (8 + 4 * 64 + 64 * 64 + 64) + 64 * 68                    # bytes of one stream's state
    assert torch.equal(gate.ws[per:2 * per], before[per:2 * per]) and not torch.equal(gate.ws[:per], before[:per])
    for s, lag in ((0, 0), (2, 2)):
        w = SequenceReference(ids, -2.0, potts(3, 0.5, 0.5, 0.5), lag).run_rows(lg[10 * s:10 * s + 10])
        assert_same([out[i, 10 * s:10 * s + 10] for i in range(3)], w, s)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. behind the decoders: without costs and thresholds, now is the decoder's pred
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


def recordings(n, seed, length=3000):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((rng.standard_normal((length, 12)) * (1 + 0.2 * i) * 2e-3).astype(F)).cuda() for i in range(n)]


@pytest.fixture(scope="module")
def norm():
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    w = preprocess_segments(recordings(1, 5)[0][None], keep=20 * np.arange(140))[0]
    return w.mean(0), w.std(0)


def assert_margins(logits, what):
    """from the data: every row's top-2 margin is at least 2^-19, so quantising cannot change its first maximum"""
    if logits.shape[1] > 1 and logits.shape[0]:
        top = logits.topk(2, dim=1).values
        margin = float((top[:, 0] - top[:, 1]).min())
        print(what, "smallest top-2 margin", margin)
        assert margin >= 2.0 ** -19, (what, margin)


def no_costs(i):
    return np.zeros((len(i) + 1, len(i) + 1), dtype=np.int32)


SUBSETS = [list(range(41)), [30, 2, 17, 5, 9], [7], list(range(0, 41, 3)), [40, 0]]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_without_costs_now_is_pred_single(engine, norm, dtype):
    from contrastiveprosthetics_amd.online import OnlineDecoder
    from contrastiveprosthetics_amd.sequence import SequenceGate
    mean, std = norm
    rec = recordings(1, 21)[0]
    rng = np.random.default_rng(2)
    for classes, lag in zip(SUBSETS, (0, 5, 0, 63, 1)):
        dec = OnlineDecoder(engine, mean, std, classes=classes, dtype=dtype)
        gate = SequenceGate(dec, transitions=no_costs, lag=lag)
        p, preds, cmds = 0, [], []
        while p < rec.shape[0]:
            n = int(rng.integers(1, 700))
            pred, voted, logits, cmd, now, lead = gate.push(rec[p:p + n], return_logits=True)
            assert_margins(logits, (dtype, len(classes), p))
            assert torch.equal(now, pred), (classes, p)
            assert len(gate.push(rec[:0])) == 5                        # an empty push: empty outputs, no launch
            preds.append(pred)
            cmds.append(cmd)
            p += n
        pred, cmd = torch.cat(preds), torch.cat(cmds)
        assert pred.shape[0] == 150 and (cmd[:lag] == -1).all() and torch.equal(cmd[lag:], pred[:150 - lag])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_without_costs_now_is_pred_multi(engine, norm, dtype):
    from contrastiveprosthetics_amd.online import MultiStreamDecoder
    from contrastiveprosthetics_amd.sequence import SequenceGate
    mean, std = norm
    S = len(SUBSETS) + 1                                               # the last stream never gets classes or samples
    recs = recordings(S - 1, 31)
    dec = MultiStreamDecoder(engine, mean, std, S, vote=9, dtype=dtype, max_windows_per_push=16, max_rows=40)
    for s, classes in enumerate(SUBSETS):
        dec.set_classes(s, classes=classes)
    gate = SequenceGate(dec, transitions=no_costs, lag=[0, 1, 2, 3, 4, 5])
    rng = np.random.default_rng(3)
    pos = np.zeros(S - 1, dtype=np.int64)
    rows = 0
    while (pos < 3000).any():
        n = np.minimum(rng.integers(1, 500, S - 1) * (rng.random(S - 1) > 0.3), 3000 - pos)      # (the small decoder splits these)
        chunks = [recs[s][pos[s]:pos[s] + n[s]] if n[s] or s % 2 else None for s in range(S - 1)] + [None]
        out = gate.push(chunks, return_logits=True)
        for s in range(S - 1):
            pred, voted, logits, cmd, now, lead = out[s]
            assert_margins(logits, (dtype, s, int(pos[s])))
            assert torch.equal(now, pred), (s, pos)
            rows += pred.shape[0]
        assert out[S - 1][3].shape == (0,)
        pos += n
    assert rows == 150 * (S - 1)
    from contrastiveprosthetics_amd import _lib
    dec.push([recs[0][:40]] + [None] * (S - 1))                        # behind the stage's back:
    with pytest.raises(_lib.CpNativeError):
        gate.push([recs[0][:40]] + [None] * (S - 1))                   # the next push through it raises


def test_the_smallest_margins_of_the_recordings():
    """recording(K): the smallest top-2 margin of a row, measured once and checked here"""
    for K, least in ((5, 2.3e-4), (41, 2.5e-4), (64, 1.4e-5)):
        lg = np.sort(recording(K)[1], axis=1)
        margin = float((lg[:, -1] - lg[:, -2]).min())
        assert margin >= 2.0 ** -19 and float("%.1e" % margin) == least, (K, margin)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the lowest score, and rows that are not finite
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_lowest_score_is_reached_and_held_on_the_device():
    """the case of tests/test_online_sequence_host.py (its docstring says why -2^29 itself is out of reach): scores fall to
    -2^28 - 2^22, stay there and follow the rise"""
    from contrastiveprosthetics_amd.sequence import SequenceGate, SequenceReference, potts
    lg = floor_rows()
    C = potts(3, 0.5, 300.0, 0.5, through_rest=True)
    dev = torch.from_numpy(lg).cuda()
    for lag in (0, 3):
        ref = SequenceReference([4, 5, 9], 2.0, C, lag)
        gate = SequenceGate(Ids([4, 5, 9]), transitions=lambda i: C, min_cosine=2.0, lag=lag)
        for a, b in ((0, 65), (65, 200), (200, 201), (201, 240)):
            assert_same([x.cpu().numpy() for x in gate.apply(dev[a:b])], ref.run_rows(lg[a:b]), (lag, a))
            assert_state(gate, ref.score, ref.ring, ref.n, (lag, a))
            if b == 200:
                assert gate.state()["score"].tolist() == [-(1 << 28) - (1 << 22)] * 3 + [0]


def test_rows_that_are_not_finite_carry_no_evidence_on_the_device():
    from contrastiveprosthetics_amd.sequence import SequenceGate, SequenceReference
    ids, lg, _ = recording(5)
    lg = lg[:300].copy()
    rng = np.random.default_rng(9)
    rows = rng.choice(300, 24, replace=False)
    lg[rows[:12], rng.integers(0, 5, 12)] = np.nan
    lg[rows[12:20], rng.integers(0, 5, 8)] = np.inf
    lg[rows[20:22]] = np.inf                                           # whole rows
    lg[rows[22:]] = -np.inf
    C = matrix("potts", 5)
    clean = want(5, "potts", 2)[0]
    for lag in (0, 2):
        ref = SequenceReference(ids, 0.25, C, lag)
        out = ref.run_rows(lg)
        if lag == 2:
            assert not np.array_equal(out[2], clean[2][:300])          # the rows matter
        gate = SequenceGate(Ids(ids), min_cosine=0.25, lag=lag)
        assert_same(run_cuts(gate, torch.from_numpy(lg).cuda(), [7] * 42 + [6]), out, lag)
        assert_state(gate, ref.score, ref.ring, ref.n, lag)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. behind the posture stage; following the decoder; driving the hand
# ---------------------------------------------------------------------------------------------------------------------------
def test_apply_on_posture_class_logits_equals_the_definition():
    from contrastiveprosthetics_amd import prototypes as P
    from contrastiveprosthetics_amd.sequence import SequenceGate, SequenceReference, potts

    class Rows(Ids):
        ws, vote = None, 25

    rng = np.random.default_rng(4)
    rid = np.sort(rng.choice(400, size=40, replace=False))
    gids = np.sort(rng.choice(90, size=13, replace=False))
    cls = np.concatenate([gids, rng.choice(gids, size=27)])[rng.permutation(40)]
    rows = rng.uniform(-0.25, 0.6, (300, 40)).astype(F)
    stage = P.PostureRows(Rows(rid), cls)
    gate = SequenceGate(stage, min_cosine=0.3, lag=4)
    got, logits = [], []
    for p in range(0, 300, 70):
        class_logits = stage.apply(torch.from_numpy(rows[p:p + 70]).cuda())[3]
        assert class_logits.shape[1] == 13
        got.append(gate.apply(class_logits))
        logits.append(class_logits.cpu().numpy())
    ref = SequenceReference(stage.class_ids, 0.3, potts(13, 0.5, 0.5, 0.5), 4)
    out = ref.run_rows(np.concatenate(logits))
    assert_same([torch.cat([g[i] for g in got]).cpu().numpy() for i in range(3)], out, "posture rows")
    assert len(set(out[0].tolist())) >= 4


def test_stage_follows_set_classes_and_thresholds_and_drives_the_hand(engine, norm):
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import GraspDrive, OnlineDecoder
    from contrastiveprosthetics_amd.sequence import SequenceGate, SequenceReference, potts
    mean, std = norm
    rec = recordings(1, 41)[0]
    dec = OnlineDecoder(engine, mean, std, classes=[5, 9, 17])
    gate = SequenceGate(dec, transitions=dict(switch=0.02, engage=0.01, release=0.01), lag=2)
    pred, voted, logits, wins, cmd, now, lead = gate.push(rec[:1000], return_logits=True, return_windows=True)
    ref = SequenceReference(dec.class_ids.cpu(), -2.0, potts(3, 0.02, 0.01, 0.01), 2)
    assert_same([x.cpu().numpy() for x in (cmd, now, lead)], ref.run_rows(logits), "first list")
    assert gate.state()["n"] == 50
    # the command drives the hand through GraspDrive.apply, as the documents say
    profile = dict(ids=np.array([5, 9, 17]), rest=np.full(12, -1.0, F), span=np.full((3, 12), 2.0, F), weight=np.ones((3, 12), np.int32),
                   low=np.full(12, -np.inf, F), high=np.full(12, np.inf, F))
    level, active, bad = GraspDrive(dec, profile=profile, follow="pred", smooth=1).apply(wins, cmd)
    assert level.shape == cmd.shape and (level[:2] == 0).all() and float(level.max()) > 0 and int(bad.max()) == 0
    dec.set_classes([2, 4, 6, 33])                                     # a new list: the stream restarts, with a 5 x 5 matrix
    pred, voted, logits, cmd, now, lead = gate.push(rec[1000:1400], return_logits=True)
    ref = SequenceReference([2, 4, 6, 33], -2.0, potts(4, 0.02, 0.01, 0.01), 2)
    assert_same([x.cpu().numpy() for x in (cmd, now, lead)], ref.run_rows(logits), "second list")
    assert (cmd[:2] == -1).all() and gate.state()["n"] == 20
    gate.set_thresholds({4: 0.5}, default=0.05)                        # restarts as well
    pred, voted, logits, cmd, now, lead = gate.push(rec[1400:1800], return_logits=True)
    ref = SequenceReference([2, 4, 6, 33], [0.05, 0.5, 0.05, 0.05], potts(4, 0.02, 0.01, 0.01), 2)
    assert_same([x.cpu().numpy() for x in (cmd, now, lead)], ref.run_rows(logits), "thresholds")
    gate.reset()
    assert gate.state()["n"] == 0 and gate.state()["score"].tolist() == [0] * 5
    gate.push(rec[:500])
    dec.push(rec[500:520])                                             # behind the stage's back
    ws = gate.ws.clone()
    with pytest.raises(_lib.CpNativeError):
        gate.push(rec[520:600])
    assert torch.equal(ws, gate.ws)
