"""The grasp command gate on the MI355X (contrastiveprosthetics_amd/online.py CommandGate, csrc/online_gate.cuh) against the
numpy restatement of its semantics (tests/test_online_gate_host.py GateReference): crafted logits that make the state machine
work, cut invariance, command == voted with every gate open on all four decoders, 256 streams in one launch, and the wrapper's
set_classes / reset / out-of-step behaviour.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from test_online_gate_host import GateReference

pytestmark = pytest.mark.gpu

F = np.float32
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# crafted logits
# ---------------------------------------------------------------------------------------------------------------------------
def thresholds(K):
    """one threshold per row, all exact in f32: 0.5, 0.5625, 0.625, 0.5, ..."""
    return (0.5 + 0.0625 * (np.arange(K) % 3)).astype(F)


def crafted(rng, K, n, thr, min_margin, scale=1):
    """(n, K) f32 logits in [-1, 1] that walk the gate through its cases: holds of one class (some windows exactly at the class's
    threshold), short bursts, rests where nothing reaches a threshold, windows with a close or tied runner-up (margin exactly at
    min_margin, below it, or 0), windows just below the threshold, stretches where two classes take turns, and a few NaN rows.  `scale` stretches the segments for
    long rings.  Everything that must compare exactly lies on a grid of 1/64."""
    lg = (rng.integers(-20, 20, (n, K)) / 64.0).astype(F)            # background: below every threshold, full of exact ties
    mm = F(min_margin)
    j = 0
    while j < n:
        kind = rng.choice(["hold", "burst", "rest", "ambiguous", "weak", "duel"], p=[0.27, 0.22, 0.2, 0.13, 0.08, 0.1])
        c = int(rng.integers(K))
        other = (c + 1 + int(rng.integers(K - 1))) % K if K > 1 else c
        length = {"hold": rng.integers(5, 60) * scale, "burst": rng.integers(1, 4), "rest": rng.integers(3, 60) * scale,
                  "ambiguous": rng.integers(1, 7), "weak": rng.integers(1, 7), "duel": rng.integers(40, 90) * scale}[kind]
        for i in range(j, min(n, j + int(length))):
            if kind == "duel":                                        # two classes (K = 1: one class and nothing) take turns at
                if rng.random() < 0.5:                                # random: the candidate keeps changing near the tie
                    lg[i, c] = F(rng.uniform(0.7, 1.0))
                elif K > 1:
                    lg[i, other] = F(rng.uniform(0.7, 1.0))
            elif kind in ("hold", "burst"):
                lg[i, c] = [F(0.875), thr[c], F(1.0), F(rng.uniform(0.7, 1.0))][int(rng.integers(4))]
            elif kind == "weak":
                lg[i, c] = thr[c] - F(1 / 64)                         # rejected by cosine
            elif kind == "ambiguous":
                if K == 1:
                    lg[i, c] = [mm - F(1.0), mm - F(1.0) - F(1 / 64)][int(rng.integers(2))]     # margin = c1 + 1: at / below
                else:
                    d = (c + 1 + int(rng.integers(K - 1))) % K
                    lg[i, c] = F(0.875)
                    lg[i, d] = [F(0.875) - mm, F(0.875) - mm + F(1 / 64), F(0.875)][int(rng.integers(3))]   # at / below / a tie
        j += int(length)
    lg[rng.random(n) < 0.01, int(rng.integers(K))] = np.nan
    return lg


# K, vote, weight, min_votes, dwell, release, rows, scale
CASES = [
    (1, 25, "count", 12, 4, 6, 3000, 1),
    (1, 1, "margin", 1, 2, 2, 2000, 1),
    (2, 25, "margin", 3, 3, 5, 3000, 1),
    (2, 1, "count", 1, 3, 2, 2000, 1),
    (2, 256, "count", 30, 5, 8, 24000, 8),
    (41, 25, "count", 4, 5, 10, 4000, 1),
    (41, 25, "margin", 2, 2, 0, 3000, 1),                              # release = 0: never release
    (41, 1, "margin", 1, 2, 3, 5000, 1),
    (64, 25, "margin", 3, 4, 6, 4000, 1),
    (64, 256, "margin", 30, 6, 0, 24000, 8),
    (64, 256, "count", 40, 4, 12, 24000, 8),
]


def case_events(vote, min_votes, release):
    """the events a configuration can produce at all: a ring of one window cannot hold a slot back for want of votes
    (min_votes is 1 there), and release = 0 never releases"""
    ev = set(GateReference.EVENTS)
    if min_votes == 1:
        ev.discard("blocked_min_votes")
    if release == 0:
        ev.discard("release")
    return ev


def case_input(i):
    K, vote, weight, min_votes, dwell, release, n, scale = CASES[i]
    rng = np.random.default_rng(100 + i)
    ids = np.sort(rng.choice(500, K, replace=False)).astype(np.int64)
    thr = thresholds(K)
    min_margin = 1.625 if K == 1 else 0.25
    lg = crafted(rng, K, n, thr, min_margin, scale)
    ref = GateReference(ids, thr, vote, min_votes, dwell, release, weight, min_margin)
    return ids, thr, min_margin, lg, ref


class Ids:
    """the part of a decoder that CommandGate.apply reads: class lists (one, or one per stream) and a sample count"""
    device = torch.device("cuda:0")
    phase = 0

    def __init__(self, ids, vote, multi=False):
        self.class_ids = [None if i is None else torch.as_tensor(i, dtype=torch.int32) for i in ids] if multi \
            else torch.as_tensor(ids, dtype=torch.int32)
        self.vote = vote
        self.n_seen = np.zeros(len(ids), dtype=np.int64) if multi else 0

    def push(self, *a, **k):
        raise AssertionError("apply() does not push the decoder")


def gate_for(ids, thr, vote, **kw):
    from contrastiveprosthetics_amd.online import CommandGate
    return CommandGate(Ids(ids, vote), min_cosine={int(i): float(t) for i, t in zip(ids, thr)}, **kw)


def run_cuts(gate, lg, cuts):
    dev = torch.from_numpy(lg).cuda()
    outs, p = [], 0
    for n in cuts:
        outs.append(gate.apply(dev[p:p + n]))
        p += n
    assert p == lg.shape[0]
    return [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(4)]


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("command", "accepted", "conf", "margin")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == F:                                               # bit-equal, NaN rows included
            g, w = g.view(np.int32), w.view(np.int32)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("i", range(len(CASES)))
def test_crafted_logits_against_the_restatement(i):
    K, vote, weight, min_votes, dwell, release, n, scale = CASES[i]
    ids, thr, min_margin, lg, ref = case_input(i)
    want = ref.run_rows(lg)
    # the input makes the state machine work: counted on the restatement, before anything is compared
    print(CASES[i], ref.events)
    for ev in sorted(case_events(vote, min_votes, release)):
        assert ref.events[ev] >= 10, (CASES[i], ev, ref.events)
    finite = np.isfinite(lg).all(axis=1)
    safe = np.where(np.isnan(lg), -np.inf, lg)
    top, k1 = safe.max(axis=1), safe.argmax(axis=1)
    assert (~finite).sum() >= 5                                                              # NaN rows
    assert (finite & (top == thr[k1])).sum() >= 10                                           # c1 exactly at its threshold
    assert (finite & (want[3] == F(min_margin)) & (want[1] >= 0)).sum() >= (10 if K > 1 else 3)     # margin exactly at min_margin
    if K > 1:
        assert (finite & (want[3] == 0)).sum() >= 10                                         # exact ties of the maximum
    gate = gate_for(ids, thr, vote, min_margin=min_margin, min_votes=min_votes, dwell=dwell, release=release, weight=weight)
    got = run_cuts(gate, lg, [n])
    assert_same(got, want, CASES[i])
    st = gate.state()
    assert st == ref.state(), CASES[i]


def test_set_changes_the_settings_between_pushes():
    ids, thr, min_margin, lg, ref = case_input(5)
    gate = gate_for(ids, thr, 25, min_margin=min_margin, min_votes=4, dwell=5, release=10)
    got = [run_cuts(gate, lg[:1500], [1500])]
    want = [ref.run_rows(lg[:1500])]
    gate.set(dwell=2, release=0, min_margin=0.125, min_votes=2, weight="margin")
    ref.dwell, ref.release, ref.min_margin, ref.min_votes, ref.weight = 2, 0, F(0.125), 2, "margin"
    got.append(run_cuts(gate, lg[1500:], [lg.shape[0] - 1500]))
    want.append(ref.run_rows(lg[1500:]))
    for g, w in zip(got, want):
        assert_same(g, w, "set")
    assert gate.state() == ref.state()


@pytest.mark.parametrize("i", [2, 5, 9])
def test_outputs_and_state_do_not_depend_on_the_cut(i):
    ids, thr, min_margin, lg, ref = case_input(i)
    K, vote, weight, min_votes, dwell, release, n, scale = CASES[i]
    lg = lg[:1500]
    n = lg.shape[0]
    want = ref.run_rows(lg)
    rng = np.random.default_rng(7)
    rand = []
    while sum(rand) < n:
        rand.append(int(min(rng.integers(1, 300), n - sum(rand))))
    cuts = {"1": [1] * n, "16": [16] * (n // 16) + ([n % 16] if n % 16 else []), "256": [256] * (n // 256) + [n % 256],
            "whole": [n], "random": rand}
    states = {}
    for name, c in cuts.items():
        gate = gate_for(ids, thr, vote, min_margin=min_margin, min_votes=min_votes, dwell=dwell, release=release, weight=weight)
        assert_same(run_cuts(gate, lg, c), want, (CASES[i], name))
        assert gate.state() == ref.state(), name
        states[name] = gate.ws.cpu().numpy().copy()
    for name in cuts:
        assert np.array_equal(states[name], states["1"]), name            # the whole workspace, byte for byte


# ---------------------------------------------------------------------------------------------------------------------------
# behind the decoders
# ---------------------------------------------------------------------------------------------------------------------------
def _engine(seed=3, steps=3):
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=False, dtype="f32", device="cuda:0", seed=seed)
    e.init_parameters(seed)
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(41).repeat(4).cuda()
    for _ in range(steps):
        x = (torch.randn(4 * 41, 12, generator=g) * 1.5 + 0.3).cuda()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(PARAMS)
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def engine():
    return _engine()


def _recordings(n, seed=11, length=3000):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((rng.standard_normal((length, 12)) * (1 + 0.2 * i) * 2e-3).astype(np.float32)).cuda()
            for i in range(n)]


@pytest.fixture(scope="module")
def norm():
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rec = _recordings(1, seed=5)[0]
    w = preprocess_segments(rec[None], keep=20 * np.arange(140))[0]
    return w.mean(0), w.std(0)


SUBSETS = [list(range(41)), [30, 2, 17, 5, 9], [7], list(range(0, 41, 3)), [40, 0]]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("adapt", [None, 0.01])
def test_every_gate_open_command_is_voted_single(engine, norm, dtype, adapt):
    from contrastiveprosthetics_amd.online import CommandGate, OnlineDecoder
    mean, std = norm
    rec = _recordings(1, seed=21)[0]
    rng = np.random.default_rng(2)
    for classes, vote in zip(SUBSETS, (25, 7, 3, 1, 256)):
        dec = OnlineDecoder(engine, mean, std, classes=classes, vote=vote, dtype=dtype, adapt=adapt)
        gate = CommandGate(dec)
        p, n_rows = 0, 0
        while p < rec.shape[0]:
            n = int(rng.integers(1, 700))
            pred, voted, logits, cmd, acc, conf, margin = gate.push(rec[p:p + n], return_logits=True)
            assert torch.equal(cmd, voted) and torch.equal(acc, pred), (classes, vote, p)
            assert torch.equal(conf, logits.max(dim=1).values)
            assert len(gate.push(rec[:0])) == 6                        # an empty push: empty outputs, no launch
            p += n
            n_rows += pred.shape[0]
        assert n_rows == 150


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("adaptive", [False, True])
def test_every_gate_open_command_is_voted_multi(engine, norm, dtype, adaptive):
    from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, CommandGate, MultiStreamDecoder
    mean, std = norm
    S = len(SUBSETS) + 1                                               # the last stream never gets classes or samples
    recs = _recordings(S - 1, seed=31)
    if adaptive:
        dec = AdaptiveMultiStreamDecoder(engine, mean, std, S, [0.0, 0.01, 0.02, 0.0, 0.05, 0.01], vote=9, dtype=dtype)
    else:
        dec = MultiStreamDecoder(engine, mean, std, S, vote=9, dtype=dtype, max_windows_per_push=16, max_rows=40)
    for s, classes in enumerate(SUBSETS):
        dec.set_classes(s, classes=classes)
    gate = CommandGate(dec)
    rng = np.random.default_rng(3)
    pos = np.zeros(S - 1, dtype=np.int64)
    rows = 0
    while (pos < 3000).any():
        n = np.minimum(rng.integers(1, 500, S - 1) * (rng.random(S - 1) > 0.3), 3000 - pos)      # (the small decoder splits these)
        chunks = [recs[s][pos[s]:pos[s] + n[s]] if n[s] or s % 2 else None for s in range(S - 1)] + [None]
        out = gate.push(chunks)
        for s in range(S - 1):
            pred, voted, cmd, acc, conf, margin = out[s]
            assert torch.equal(cmd, voted) and torch.equal(acc, pred), (s, pos)
            rows += pred.shape[0]
        assert out[S - 1][2].shape == (0,)
        pos += n
    assert rows == 150 * (S - 1)
    raw = torch.cat([r[:40] for r in recs])
    dec.reset()
    gate.reset()
    out = gate.push_packed(raw, [40] * (S - 1) + [0], return_logits=True)
    assert all(torch.equal(o[3], o[1]) and o[2].shape[1] == len(c) for o, c in zip(out, SUBSETS))


def test_256_streams_in_one_launch_each_equal_their_own_gate():
    from contrastiveprosthetics_amd.online import CommandGate
    rng = np.random.default_rng(5)
    S, launches = 256, 12
    ks = rng.choice([1, 2, 3, 5, 17, 41, 64], S)
    ids = [np.sort(rng.choice(300, k, replace=False)) for k in ks]
    thr = [(rng.integers(16, 44, k) / 64.0).astype(F) for k in ks]
    cfg = dict(min_margin=0.125, min_votes=2, dwell=3, release=4, weight="margin")
    many = CommandGate(Ids(ids, 25, multi=True), **cfg)
    for s in range(S):
        many.set_thresholds(s, {int(i): float(t) for i, t in zip(ids[s], thr[s])})
    m = rng.integers(0, 13, (launches, S)) * (rng.random((launches, S)) > 0.25)          # some streams sit a launch out
    m[:, 7] = 0                                                                         # and one never has a row
    total = m.sum(axis=0)
    lgs = [crafted(rng, int(ks[s]), int(total[s]), thr[s], 0.125) if total[s] else np.zeros((0, int(ks[s])), F) for s in range(S)]
    dev = [torch.from_numpy(x).cuda() for x in lgs]
    pos = np.zeros(S, dtype=np.int64)
    got = [[] for _ in range(S)]
    for r in range(launches):
        packed = torch.full((int(m[r].sum()), 64), float("nan"), device="cuda")       # as a multi-stream push packs them:
        row0 = np.concatenate([[0], np.cumsum(m[r])[:-1]])                             # columns past K_s are never read
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
        g = [torch.cat([o[i] for o in got[s]]).cpu().numpy() for i in range(4)]
        ref = GateReference(ids[s], thr[s], 25, min_margin=0.125, min_votes=2, dwell=3, release=4, weight="margin")
        want = ref.run_rows(lgs[s])
        assert_same(g, want, ("restatement", s, int(ks[s])))
        own = gate_for(ids[s], thr[s], 25, **cfg)
        if total[s]:
            assert_same(g, run_cuts(own, lgs[s], [int(total[s])]), ("own gate", s))
        assert many.state(s) == own.state() == ref.state(), s
    assert many.state(7) == dict(command=-1, pending=None, run=0, ring=[])


def test_separately_allocated_logits_are_packed_for_the_launch():
    """apply() on tensors that are not one packed buffer (the caller's own, or a push the decoder split) takes the copy path"""
    from contrastiveprosthetics_amd.online import CommandGate
    rng = np.random.default_rng(8)
    ids = [np.array([1, 5, 9]), None, np.arange(41)]
    gate = CommandGate(Ids(ids, 5, multi=True), min_cosine=0.5, dwell=2)
    lgs = [crafted(rng, 3, 700, thresholds(3) * 0 + F(0.5), 0.0), None, crafted(rng, 41, 300, thresholds(41) * 0 + F(0.5), 0.0)]
    out = gate.apply([None if x is None else torch.from_numpy(x).cuda() for x in lgs])     # 700 rows: three launches
    for s in (0, 2):
        ref = GateReference(ids[s], 0.5, 5, dwell=2)
        assert_same([o.cpu().numpy() for o in out[s]], ref.run_rows(lgs[s]), s)
    assert out[1][0].shape == (0,)


def test_wrapper_follows_set_classes_reset_and_refuses_a_push_behind_its_back(engine, norm):
    from contrastiveprosthetics_amd._lib import CpNativeError
    from contrastiveprosthetics_amd.online import CommandGate, OnlineDecoder
    mean, std = norm
    rec = _recordings(1, seed=41)[0]
    dec = OnlineDecoder(engine, mean, std, classes=[3, 8, 20], vote=25)
    gate = CommandGate(dec, dwell=2)
    out = gate.push(rec[:1000])
    cmd = int(out[2][-1])
    st = gate.state()
    assert cmd in (3, 8, 20) and st["command"] == cmd and len(st["ring"]) == 25
    dec.set_classes([cmd, 33, 1])                                       # the command's id survives: kept; the ring is empty
    out = gate.push(rec[1000:1020])
    st = gate.state()
    assert out[2].shape == (1,) and len(st["ring"]) == 1
    assert int(out[2][0]) == cmd                                        # (dwell = 2: one window cannot replace it)
    gate.push(rec[1020:1400])
    assert gate.state()["command"] in (cmd, 33, 1)
    dec.set_classes([2, 4, 6])                                          # its id is gone: the command becomes none
    out = gate.push(rec[1400:1420])
    assert int(out[2][0]) == -1 and gate.state()["command"] == -1 and len(gate.state()["ring"]) == 1
    gate.push(rec[1420:2000])
    assert gate.state()["command"] in (2, 4, 6)
    gate.reset()
    assert dec.n_seen == 0 and gate.state() == dict(command=-1, pending=None, run=0, ring=[])
    gate.push(rec[:500])
    dec.push(rec[500:520])                                              # behind the gate's back
    before = gate.state()
    with pytest.raises(CpNativeError, match="behind"):
        gate.push(rec[520:600])
    assert dec.n_seen == 520 and gate.state() == before                 # nothing was enqueued
    gate.reset()
    assert len(gate.push(rec[:100])[2]) == 5


def test_thresholds_from_a_cued_recording_reject_rest(engine, norm):
    """thresholds_from_logits pairs with window_labels and a push of the recording: on its own recording about `keep` of the
    correct windows of each class pass their class's threshold"""
    from contrastiveprosthetics_amd.online import CommandGate, OnlineDecoder, thresholds_from_logits, window_labels
    mean, std = norm
    rec = _recordings(1, seed=51, length=6000)[0]
    classes = [1, 4, 6, 30]
    dec = OnlineDecoder(engine, mean, std, classes=classes)
    pred, voted, logits = dec.push(rec, return_logits=True)
    labels = np.repeat(pred.cpu().numpy().astype(np.int64), 20)[:6000]  # cue every sample with what its window decodes as
    labels = np.concatenate([labels, np.full(6000 - labels.shape[0], -1)])
    wl = window_labels(labels)
    thr = thresholds_from_logits(logits, wl, dec.class_ids, keep=0.8)
    assert set(thr) <= set(classes) and thr
    dec.reset()
    gate = CommandGate(dec, min_cosine=thr, default=2.0)                # classes without a threshold never pass
    out = gate.push(rec)
    acc, conf = out[3].cpu().numpy(), out[4].cpu().numpy()
    p = pred.cpu().numpy()
    for c, t in thr.items():
        sel = p == c
        assert np.array_equal(acc[sel] == c, conf[sel] >= F(t))
        ok = (wl == c) & sel
        if ok.sum() >= 20:
            assert 0.7 <= (acc[ok] == c).mean() <= 0.9, (c, (acc[ok] == c).mean())
    assert (acc[~np.isin(p, list(thr))] == -1).all()
