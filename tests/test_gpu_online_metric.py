"""The user metric on the MI355X (contrastiveprosthetics_amd/metric.py fit_metric, Metric.apply, MetricRows, pick_shrink and
metric_enrolment, csrc/online_metric.cuh) against the numpy definitions `fit_reference`, `apply_reference` and
`stage_reference`: moments, counts, A and valid in every bit, the transform, the stage in every integer and bit, cut and
neighbour invariance, the stage behind the four decoders, and the chain from a recording to the gate.  Every comparison is
exact; the payload bits of a NaN are the one thing not compared (the definition does not set them)."""
import ctypes

import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import metric as M
from contrastiveprosthetics_amd._lib import CpNativeError
from test_gpu_online_track import KINDS, _recordings, chunks_of, engine, make_decoder, norm, same_floats  # noqa: F401 (fixtures)
from test_online_metric_host import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
R, I = M.REST, M.IGNORE
EYE = np.eye(16, dtype=F)
M_SET = (1, 15, 16, 17, 63, 64, 65, 700)


class Source:
    """the part of a decoder that MetricRows.apply reads: class lists, a sample count, a vote length and a device"""
    device = torch.device("cuda:0")
    phase, ws = 0, None

    def __init__(self, vote, n_streams=None):
        self.class_ids = None if n_streams is None else [None] * n_streams
        self.n_seen = 0 if n_streams is None else np.zeros(n_streams, dtype=np.int64)
        self.vote = vote

    def push(self, *a, **k):
        raise AssertionError("apply() does not push the decoder")


# ---------------------------------------------------------------------------------------------------------------------------
# the fit against the definition
# ---------------------------------------------------------------------------------------------------------------------------
def fit_case(m, k, seed, wide=False):
    """a recording of m windows over k class ids that has what the fit must get right: one loud axis, duplicate windows,
    IGNORE and REST windows, a class that is absent, one with three windows, a NaN, an Inf and an all-zero window; wide: the
    components are spread over 40 binary orders of magnitude, so that the order of every sum shows in its bits"""
    rng = np.random.default_rng(seed)
    ids = np.arange(k) * 3 + 2
    centres = rng.standard_normal((k, 16))
    loud = rng.standard_normal(16)
    present = np.arange(k) if k < 3 else np.delete(np.arange(k), k // 2)       # class k // 2 never appears
    slot = rng.choice(present, size=m)
    if k >= 3 and m >= 64:
        rare = present[-1]
        slot[slot == rare] = present[0]
        slot[rng.choice(m, size=3, replace=False)] = rare                      # three windows: below min_windows
    emb = centres[slot] + rng.standard_normal((m, 1)) * loud + 0.3 * rng.standard_normal((m, 16))
    emb = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    if wide:
        emb = emb * np.exp2(rng.integers(-20, 21, size=(m, 16)))
    emb = emb.astype(F)
    exp = ids[slot].astype(np.int64)
    if m >= 15:
        emb[m // 2:m // 2 + 4] = emb[1]                        # duplicates
        exp[m // 2:m // 2 + 4] = exp[1]
        exp[3], exp[m - 2] = I, R
        emb[5, 7], emb[6, 0], emb[8] = np.nan, np.inf, 0.0
    if m >= 700:
        emb[rng.choice(m, size=40, replace=False), rng.integers(0, 16, size=40)] = np.nan
        exp[rng.choice(m, size=60, replace=False)] = rng.choice([R, I], size=60)
    return emb, exp, ids


def shrinks_of(n):
    return {1: (0.3,), 5: (0.0, 1.0, 0.5, 0.1, 0.01), 64: tuple(np.linspace(0.0, 1.0, 64).tolist())}[n]


def assert_fit(got: M.Metric, want: dict, what):
    assert same_bits(got.counts, want["counts"]), (what, "counts", got.counts, want["counts"])
    assert same_bits(got.valid, want["valid"]), (what, "valid", got.valid, want["valid"])
    assert same_bits(got.moments.cpu().numpy(), want["moments"]), (what, "moments")
    assert same_bits(got.A.cpu().numpy(), want["A"]), (what, "A")
    assert same_bits(got.shrinks, want["shrinks"]) and same_bits(got.ids, want["ids"])


FIT_CASES = [  # m, k, shrink values, min_windows, use
    (1, 1, 1, 1, False), (15, 2, 5, 1, False), (16, 1, 5, 1, True), (17, 2, 64, 2, False), (63, 2, 5, 3, True), (64, 16, 1, 1, False),
    (65, 16, 5, 2, True), (65, 64, 1, 1, False), (700, 1, 5, 5, False), (700, 2, 64, 25, True), (700, 16, 5, 4, True),
    (700, 41, 5, 4, False), (700, 64, 5, 4, True),
]


@pytest.mark.parametrize("m,k,n_shrinks,minw,masked", FIT_CASES)
def test_fit_equals_the_definition(m, k, n_shrinks, minw, masked):
    emb, exp, ids = fit_case(m, k, seed=m + k)
    use = (np.random.default_rng(m).random(m) < 0.8) if masked else None
    lam = shrinks_of(n_shrinks)
    want = M.fit_reference(emb, exp, ids, lam, minw, use)
    print(m, k, n_shrinks, minw, masked, "valid", int(want["valid"].sum()), "of", len(lam), "counts", want["counts"].tolist()[:6])
    got = M.fit_metric(torch.from_numpy(emb).cuda(), exp, ids, lam, minw, use)
    assert_fit(got, want, (m, k, n_shrinks, minw, masked))
    if 1.0 in lam and want["valid"].any():
        assert same_bits(got.A.cpu().numpy()[lam.index(1.0)], EYE)


def test_fit_input_covers_the_hard_cases_and_a_class_does_not_depend_on_the_others():
    emb, exp, ids = fit_case(700, 16, seed=9)
    want = M.fit_reference(emb, exp, ids, shrinks_of(5), 4)
    # asserted on the definition: short and absent classes, windows that do not train, valid and invalid shrink values
    assert (want["counts"] == 0).sum() == 1 and (want["counts"] == 3).sum() == 1 and (want["counts"] >= 4).sum() == 14
    assert want["valid"].tolist() == [True] * 5 and not np.isfinite(emb).all() and (exp == I).any() and (exp == R).any()
    flat = M.fit_reference(emb[:40], exp[:40], ids, shrinks_of(5), 4)
    assert flat["valid"].tolist() != [True] * 5                 # forty windows over fifteen classes: not every value factors
    dev = torch.from_numpy(emb).cuda()
    assert_fit(M.fit_metric(dev, exp, ids, shrinks_of(5), 4), want, "full")
    assert_fit(M.fit_metric(dev[:40], exp[:40], ids, shrinks_of(5), 4), flat, "forty")
    for c in (0, 5, 15):
        alone = M.fit_metric(dev, np.where(exp == ids[c], exp, R), [int(ids[c])], (0.5,), 4)
        assert same_bits(alone.moments.cpu().numpy()[0], want["moments"][c]) and alone.counts[0] == want["counts"][c]


def test_every_sum_runs_in_window_order():
    emb, exp, ids = fit_case(700, 4, seed=4, wide=True)         # three classes with windows, the last with three
    fwd, cnt = M.moments_reference(emb, exp, ids)
    keep = np.isfinite(emb).all(axis=1) & (exp >= 0)
    rev, _ = M.moments_reference(emb[keep][::-1], exp[keep][::-1], ids)
    differs = fwd != rev
    print("entries whose bits depend on the order:", int(differs.sum()), "of", differs.size, "counts", cnt.tolist())
    assert differs[:, :16].any() and differs[:, 16:].any() and (cnt >= 2).sum() == 3
    lam = shrinks_of(5)
    want = M.fit_reference(emb, exp, ids, lam, 2)
    assert want["valid"].any()
    assert_fit(M.fit_metric(torch.from_numpy(emb).cuda(), exp, ids, lam, 2), want, "wide")
    # the classes the other way round: the same moments in the other slots, pooled in the other order
    mirrored = np.where(exp >= 0, ids[0] + ids[3] - exp, exp)
    other = M.fit_reference(emb, mirrored, ids, lam, 2)
    assert same_bits(other["moments"], want["moments"][::-1])
    assert_fit(M.fit_metric(torch.from_numpy(emb).cuda(), mirrored, ids, lam, 2), other, "mirrored")


def test_slots_outside_the_classes_train_nothing():
    from contrastiveprosthetics_amd import _lib
    emb, exp, ids = fit_case(700, 16, seed=2)
    slots = np.searchsorted(ids, np.where(exp >= 0, exp, ids[0])).astype(np.int32)
    slots[exp < 0] = -1
    wild = slots.copy()
    rng = np.random.default_rng(0)
    at = rng.choice(700, size=50, replace=False)
    wild[at] = rng.choice([16, 17, 64, 1000, 2 ** 31 - 1, -2, -5, -2 ** 31], size=50)
    want, cnt = M.moments_reference(emb, np.where(np.isin(np.arange(700), at), R, exp), ids)
    lib = _lib.load()
    dev, slot_d = torch.from_numpy(emb).cuda(), torch.from_numpy(wild).cuda()
    mom = torch.empty(16, 152, dtype=torch.float64, device="cuda")
    counts = torch.empty(16, dtype=torch.int64, device="cuda")
    _lib.check(lib.cp_online_metric_moments(dev.data_ptr(), 700, 16, slot_d.data_ptr(), None, mom.data_ptr(), counts.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "cp_online_metric_moments")
    assert same_bits(mom.cpu().numpy(), want) and same_bits(counts.cpu().numpy(), cnt)
    # counts the factor cannot use (negative, or below min_windows everywhere) leave the identity and valid = 0
    a = torch.empty(2, 16, 16, dtype=torch.float32, device="cuda")
    valid = torch.empty(2, dtype=torch.uint8, device="cuda")
    bad = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.cp_online_metric_factor(mom.data_ptr(), bad.data_ptr(), 16, 4, (ctypes.c_double * 2)(0.5, 1.0), 2, a.data_ptr(),
                                           valid.data_ptr(), torch.cuda.current_stream().cuda_stream), "cp_online_metric_factor")
    assert valid.cpu().tolist() == [0, 0] and same_bits(a.cpu().numpy(), np.stack([EYE, EYE]))


# ---------------------------------------------------------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def metric():
    """a fitted metric shared by the tests below: shrink 1 (the identity), 0.1 and 0.01"""
    emb, exp = M.metric_recording(1500, 4, seed=0)
    fit = M.fit_reference(emb, exp, np.arange(4), (1.0, 0.1, 0.01), min_windows=10)
    assert fit["valid"].all()
    for a in fit["A"]:
        a.setflags(write=False)
    return M.Metric.of(fit)


@pytest.mark.parametrize("m", M_SET)
def test_apply_equals_the_definition(metric, m):
    emb, _, _ = fit_case(m, 2, seed=m, wide=m == 700)
    if m >= 15:
        emb[2, 3] = -0.0
    dev = torch.from_numpy(emb).cuda()
    for t in range(3):
        want = M.apply_reference(emb, metric.A[t])
        got = metric.apply(dev, t).cpu().numpy()
        assert same_floats(got, want), (m, t)
        if 15 <= m < 700:                                      # (the long recording has NaNs of its own among the first rows)
            assert not np.isfinite(want[[5, 6, 8]]).all(axis=1).any() and np.isfinite(want[:5]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the stage against the definition
# ---------------------------------------------------------------------------------------------------------------------------
def stage_case(n, k, seed):
    """n unit embeddings around k class rows with ties (a duplicate row), signed zeros and windows that are not finite"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(500, size=k, replace=False)).astype(np.int64)
    rows = rng.standard_normal((k, 16)) * rng.uniform(0.5, 2.0, size=(k, 1))   # not unit: the stage normalises
    if k >= 2:
        rows[k - 1] = rows[0]                                  # a tie in every window: the smaller slot
    emb = rows[rng.integers(0, k, size=n)] + 0.8 * rng.standard_normal((n, 16))
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(F)
    rows = rows.astype(F)
    for r, c, v in [(7, 3, np.nan), (40, 0, np.inf), (41, None, 0.0), (50, 15, -np.inf), (51, 2, np.nan), (60, 4, -0.0), (61, None, -0.0)]:
        if r < n:
            if c is None:
                emb[r] = v
            else:
                emb[r, c] = v
    return emb, rows, ids


def apply_cuts(stage, emb, cuts):
    dev = torch.from_numpy(emb).cuda()
    outs, p = [], 0
    for n in cuts:
        outs.append(stage.apply(dev[p:p + n], return_logits=True))
        p += n
    assert p == emb.shape[0]
    return [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(3)]


def assert_stage(got, want, what):
    pred, voted, logits = got
    for name, g in (("pred", pred), ("voted", voted)):
        bad = np.nonzero(g.astype(np.int64) != want[name])[0]
        assert g.dtype == np.int32 and bad.size == 0, (what, name, bad[:5], g[bad[:5]], want[name][bad[:5]])
    assert same_floats(logits, want["logits"]), (what, "logits")


def slots_of(pred, ids):
    return [-1 if p < 0 else int(np.searchsorted(ids, p)) for p in pred.tolist()]


@pytest.mark.parametrize("windows", [1, 25, 256])
@pytest.mark.parametrize("vote", [1, 25, 256])
@pytest.mark.parametrize("K", [1, 2, 41, 64])
def test_stage_equals_the_definition(metric, K, vote, windows):
    n = 600 if windows > 1 else 90
    emb, rows, ids = stage_case(n, K, seed=K + vote)
    cuts = [windows] * (n // windows) + ([n % windows] if n % windows else [])
    for t in (0, 1):                                           # the identity, where duplicate rows tie bit for bit, and a metric
        want = M.stage_reference(emb, metric.A[t], rows, ids, vote=vote)
        assert (want["pred"] == -1).sum() >= 4 and (K <= 2 or len(set(want["pred"].tolist())) > 2)
        assert K < 2 or not (want["pred"] == ids[-1]).any()    # the duplicate of row 0 never wins
        stage = M.MetricRows(Source(vote), metric, rows, ids, t)
        assert_stage(apply_cuts(stage, emb, cuts), want, (K, vote, windows, t))
        st = stage.state()
        assert st["ids"] == ids.tolist() and st["has_metric"] == 1 and stage.class_ids.tolist() == ids.tolist()
        assert st["ring"] == slots_of(want["pred"], ids)[-vote:]
        assert same_bits(st["rows"], H._unit_rows(rows)) and same_bits(st["A"], np.tril(metric.A[t]))


def test_a_row_that_is_not_finite_silences_the_stage(metric):
    emb, rows, ids = stage_case(90, 5, seed=1)
    rows[2] = 0.0                                              # its unit row is 0 / 0
    want = M.stage_reference(emb, metric.A[1], rows, ids, vote=5)
    assert (want["pred"] == -1).all() and (want["voted"] == -1).all() and np.isnan(want["logits"][:, 2]).all()
    assert_stage(apply_cuts(M.MetricRows(Source(5), metric, rows, ids, 1), emb, [90]), want, "zero row")


def test_any_cut_gives_the_same_outputs_and_state(metric):
    emb, rows, ids = stage_case(1020, 40, seed=3)
    want = M.stage_reference(emb, metric.A[2], rows, ids, vote=25)
    states = []
    for cut in (1020, 1, 7, 64, 255):
        stage = M.MetricRows(Source(25), metric, rows, ids, 2)
        got = apply_cuts(stage, emb, [cut] * (1020 // cut) + ([1020 % cut] if 1020 % cut else []))
        assert_stage(got, want, cut)
        states.append(stage.ws.cpu().numpy().tobytes())
    assert all(s == states[0] for s in states)


def test_three_streams_with_their_own_metrics_share_a_launch_and_idle_streams_stay(metric):
    from contrastiveprosthetics_amd import _lib
    cases = [stage_case(300, 64, seed=1), stage_case(300, 7, seed=2), stage_case(300, 30, seed=3)]
    stage = M.MetricRows(Source(25, 5))                        # stream 3 never gets a metric, stream 4 a metric without rows
    for s, (_, rows, ids) in enumerate(cases):
        assert metric.install(stage.decoder, torch.from_numpy(rows).cuda(), ids, s, stream=s, stage=stage) is stage
    dev = [torch.from_numpy(c[0]).cuda() for c in cases]
    outs, p = [], 0
    for n in (1, 64, 200, 35):                                 # stream 1 sits the second launch out
        sit = n == 64
        before = stage.state(1) if sit else None
        outs.append(stage.apply([dev[0][p:p + n], None if sit else dev[1][p:p + n], dev[2][p:p + n], None, None], return_logits=True))
        if sit:
            after = stage.state(1)
            assert after["ring"] == before["ring"] and same_bits(after["rows"], before["rows"]) and outs[-1][1][0].shape == (0,)
        assert outs[-1][3] is None and outs[-1][4] is None
        p += n
    assert stage.state(3)["ring"] == [] and stage.state(3)["has_metric"] == 0 and stage.state(3)["ids"] == []
    for s, (emb, rows, ids) in enumerate(cases):
        if s == 1:                                             # its own windows, in its own order
            emb = np.concatenate([emb[:1], emb[65:300]])
        want = M.stage_reference(emb, metric.A[s], rows, ids, vote=25)
        got = [torch.cat([o[s][i] for o in outs]).cpu().numpy() for i in range(3)]
        assert_stage(got, want, s)
        alone = M.MetricRows(Source(25), metric, rows, ids, s)
        assert_stage(apply_cuts(alone, emb, [emb.shape[0]]), want, (s, "alone"))
    with pytest.raises(CpNativeError, match="no metric"):
        stage.apply([None, None, None, dev[0][:3], None])
    # the launch itself: a stream without a metric, one with a metric and no rows, and one whose rows leave the buffer are
    # left untouched, outputs and state, next to a stream that decodes
    lib, cur = stage.lib, torch.cuda.current_stream().cuda_stream
    a_d = torch.from_numpy(np.ascontiguousarray(metric.A[1])).cuda()
    _lib.check(lib.cp_online_metric_set(25, 5, stage.ws.data_ptr(), stage.ws.numel(), 4, a_d.data_ptr(), None, None, 0, cur), "set")
    torch.cuda.synchronize()
    assert stage.state(4)["has_metric"] == 1 and stage.state(4)["ids"] == []
    before = stage.ws.cpu().numpy().copy()
    words = M._OM_WORDS * 4
    for row0, m in (([0, 10, 20, 30, 40], [10, 10, 10, 10, 10]), ([0, 10, 45, 30, 40], [10, 257, 10, 10, 10]),
                    ([0, -1, 2 ** 31 - 1, 30, 40], [10, 10, 10, 10, 10]), ([0, 10, 20, 30, 40], [10, -3, 0, 10, 10])):
        rm = torch.tensor([row0, m], dtype=torch.int32, device="cuda")
        pv = torch.full((2, 50), -9, dtype=torch.int32, device="cuda")
        lg = torch.full((50, 64), -9.0, dtype=torch.float32, device="cuda")
        _lib.check(lib.cp_online_metric_push(25, 5, stage.ws.data_ptr(), stage.ws.numel(), dev[0].data_ptr(), rm[0].data_ptr(),
                                             rm[1].data_ptr(), 50, pv[0].data_ptr(), pv[1].data_ptr(), lg.data_ptr(), 64, cur), "push")
        torch.cuda.synchronize()
        after = stage.ws.cpu().numpy()
        live = [s for s in range(3) if 1 <= m[s] <= 256 and 0 <= row0[s] <= 50 - m[s]]
        assert 0 in live
        for s in range(5):
            lo, hi = (row0[s], row0[s] + m[s]) if s in live else (0, 0)
            if s in live:
                assert (pv[:, lo:hi] != -9).all() and (lg[lo:hi, :cases[s][2].shape[0]] != -9).all(), (row0, m, s)
            else:
                assert same_bits(after[s * words:(s + 1) * words], before[s * words:(s + 1) * words]), (row0, m, s)
        written = np.zeros(50, dtype=bool)
        for s in live:
            written[row0[s]:row0[s] + m[s]] = True
        assert (pv.cpu().numpy()[:, ~written] == -9).all() and (lg.cpu().numpy()[~written] == -9).all(), (row0, m)
        before = after.copy()


# ---------------------------------------------------------------------------------------------------------------------------
# behind the decoders
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_behind_a_decoder_the_stage_equals_the_definition_and_the_decoder_is_unchanged(engine, norm, metric, kind):
    recs = _recordings(2, seed=31)
    staged, plain = make_decoder(kind, engine, norm, "f32"), make_decoder(kind, engine, norm, "f32")
    multi = kind.startswith("multi")
    # the rows: six whitened windows of the stream itself, scaled, so that the predictions move between the classes (an
    # untrained encoder's embeddings lie close together; random rows would all but one never win)
    probe = make_decoder(kind, engine, norm, "f32")
    seen = [probe.push(chunks_of(kind, recs, q, 2000), return_embeddings=True) for q in (0, 2000)]
    first = torch.cat([(r[0] if multi else r)[-1] for r in seen]).cpu().numpy()
    ids = np.array([3, 10, 11, 40, 77, 500])
    rows = (M.apply_reference(first, metric.A[1])[[5, 40, 75, 110, 145, 180]] * F(1.7)).astype(F)
    stage = M.MetricRows(staged, metric, torch.from_numpy(rows).cuda(), ids, 1, 0 if multi else None)     # stream 1 sits out
    own = []                                                 # what the staged decoder itself returned
    for name in ("push", "push_packed"):
        if hasattr(staged, name):
            def wrap(*a, _f=getattr(staged, name), **k):
                own.append(_f(*a, **k))
                return own[-1]
            setattr(staged, name, wrap)
    rng = np.random.default_rng(2)
    got, embs, p = [], [], 0
    while p < 3000:
        n = int(rng.integers(1, 900))
        a = stage.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True)
        b = plain.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True, return_embeddings=True)
        p += n
        for s, (ra, rb, ro) in enumerate(zip(a, b, own[-1]) if multi else [(a, b, own[-1])]):
            assert len(ra) == 4 and len(rb) == 5
            # the decoder's own pred, voted, (logits, where a stream passes through,) windows and embeddings are what they
            # are without the stage
            names = ("pred", "voted", "logits", "windows", "embeddings")
            theirs = dict(zip(names, rb))
            for what, x in zip(names if len(ro) == 5 else names[:2] + names[3:], ro):
                y = theirs[what]
                assert x.shape == y.shape and x.dtype == y.dtype and same_bits(x.cpu().numpy(), y.cpu().numpy()), (kind, p, s, what)
            assert same_bits(ra[3].cpu().numpy(), rb[3].cpu().numpy())
            if s == 0:
                got.append(ra)
                embs.append(rb[4])
            else:                                              # a stream without a metric: the decoder's own outputs
                for x, y, what in zip(ra, rb, ("pred", "voted", "logits")):
                    assert x.shape == y.shape and same_bits(x.cpu().numpy(), y.cpu().numpy()), (kind, p, s, what)
    emb = torch.cat(embs).cpu().numpy()
    want = M.stage_reference(emb, metric.A[1], rows, ids, vote=9)
    assert emb.shape[0] > 100 and len(set(want["pred"].tolist())) > 2
    assert_stage([torch.cat([g[i] for g in got]).cpu().numpy() for i in range(3)], want, kind)
    assert (stage.class_ids[0] if multi else stage.class_ids).tolist() == ids.tolist()
    if multi:
        assert stage.class_ids[1] is staged.class_ids[1]
        raw = torch.cat([recs[0][:400], recs[1][:100]])
        for d in (stage, plain):
            d.reset()
        a = stage.push_packed(raw, [400, 100, 0, 0], return_logits=True)
        b = plain.push_packed(raw, [400, 100, 0, 0], return_logits=True, return_embeddings=True)
        w = M.stage_reference(b[0][3].cpu().numpy(), metric.A[1], rows, ids, vote=9)
        assert_stage([x.cpu().numpy() for x in a[0]], w, (kind, "packed"))
        assert all(torch.equal(x, y) for x, y in zip(a[1], b[1][:3])) and a[2][0].shape == (0,)
    else:
        with pytest.raises(TypeError):
            stage.push_packed(recs[0][:40], [40])
    # a push of the decoder behind the stage's back is refused before anything is enqueued
    staged.push(chunks_of(kind, recs, 0, 40))
    with pytest.raises(CpNativeError, match="behind the metric stage"):
        stage.push(chunks_of(kind, recs, 40, 40))
    stage.reset()
    stage.push(chunks_of(kind, recs, 0, 40))


def _count_kernels(fn, pushes=4):
    """library kernels per call, as tools/online_bench.py count_kernels counts them"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(pushes):
            fn()
        torch.cuda.synchronize()
    n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in ev.name
            and "Memset" not in ev.name)
    return n / pushes


@pytest.mark.parametrize("kind", ["single", "multi"])
def test_the_stage_adds_one_launch_to_a_push(engine, norm, metric, kind):
    recs = _recordings(2, seed=41)
    staged, plain = make_decoder(kind, engine, norm, "f32"), make_decoder(kind, engine, norm, "f32")
    multi = kind == "multi"
    _, rows, ids = stage_case(10, 6, seed=8)
    stage = M.MetricRows(staged, metric, torch.from_numpy(rows).cuda(), ids, 1, 0 if multi else None)
    if multi:
        metric.install(staged, torch.from_numpy(rows).cuda(), ids, 2, stream=1, stage=stage)
    chunk = chunks_of(kind, recs, 0, 500)
    for d in (plain, stage):
        d.push(chunk)                                          # (the counts' device copy is made once)
    a = _count_kernels(lambda: plain.push(chunk, return_embeddings=True))
    b = _count_kernels(lambda: stage.push(chunk))
    assert b == a + 1 and a >= 10, (a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: a recording, the pick, the enrolment, the stage, the gate sweep, the gate and the drive
# ---------------------------------------------------------------------------------------------------------------------------
def test_pick_shrink_gives_the_integers_of_the_definitions():
    emb, exp = M.metric_recording(1500, 4, seed=0)
    ids = np.arange(4)
    lam = (1.0,) + M.SHRINKS
    want = M.pick_shrink_reference(emb, exp, ids, lam, min_windows=10)
    got = M.pick_shrink(torch.from_numpy(emb).cuda(), exp, ids, lam, min_windows=10)
    for key in ("voted_hit", "n_cue", "shrinks"):
        assert same_bits(got[key], want[key]), (key, got[key], want[key])
    assert got["baseline"] == want["baseline"] and got["best"] == want["best"] and got["shrink"] == want["shrink"] and got["n_rep"] == 8
    assert got["shrink"] < 1.0 and got["voted_hit"][got["best"]] > got["baseline"][0] + 200


def test_from_a_recording_to_class_commands(engine, norm):
    from contrastiveprosthetics_amd.online import CommandGate, GraspDrive, OnlineDecoder, drive_profile, sweep_gate, windows_before
    mean, std = norm
    raw = _recordings(1, seed=51, length=12400)[0]
    m = windows_before(raw.shape[0], 0)
    _, exp = M.metric_recording(m, 4, seed=0, segment=30, rest=8)              # the cue schedule of the synthetic person
    ids = np.array([0, 1, 2, 3])
    dec = OnlineDecoder(engine, mean, std, classes=[0, 1, 2, 3, 7], vote=9, dtype="f32")
    dec.push(raw[:333])                                        # a stream in progress: the enrolment leaves it as it was
    seen, ws = dec.n_seen, dec.ws[:H._state_bytes(dec, False)].clone()
    lam = (1.0, 0.5, 0.1)
    out = M.metric_enrolment(dec, raw, exp, lam, min_windows=10, ids=ids)
    assert dec.n_seen == seen and torch.equal(dec.ws[:ws.numel()], ws) and dec.class_ids.tolist() == [0, 1, 2, 3, 7]
    emb = out["embeddings"].cpu().numpy()
    assert emb.shape == (m, 16) and out["valid"].all()
    want_pick = M.pick_shrink_reference(emb, exp, ids, lam, vote=9, min_windows=10)
    for key in ("voted_hit", "n_cue"):
        assert same_bits(out["pick"][key], want_pick[key]), (key, out["pick"][key], want_pick[key])
    assert out["pick"]["baseline"] == want_pick["baseline"] and out["shrink"] == want_pick["shrink"]
    fit = M.fit_reference(emb, exp, ids, (out["shrink"],), 10)
    assert same_bits(out["metric"].A.cpu().numpy(), fit["A"]) and out["metric"].valid.tolist() == [True]
    # the rows are the shipped centre-0 path on the whitened embeddings
    from contrastiveprosthetics_amd.prototypes import fit_reference as proto_reference
    e2 = M.apply_reference(emb, fit["A"][0])
    assert same_floats(out["metric"].apply(out["embeddings"]).cpu().numpy(), e2)
    rows = proto_reference(e2, exp, ids, 1, iters=0, min_windows=10)["rows"][:, 0]
    assert same_bits(out["rows"].cpu().numpy(), rows)
    stage = out["stage"]
    assert stage.class_ids.tolist() == ids.tolist() and stage.decoder is dec
    stage.reset()
    outs, p = [], 0
    for n in (4000, 37, 2600, 5763):
        outs.append(stage.push(raw[p:p + n], return_logits=True))
        p += n
    pred, voted, logits = (torch.cat([o[i] for o in outs]) for i in range(3))
    want = M.stage_reference(emb, fit["A"][0], rows, ids, vote=9)
    assert_stage([pred.cpu().numpy(), voted.cpu().numpy(), logits.cpu().numpy()], want, "end to end")
    # what the stage decodes is what the hold-out entries score on the whitened embeddings
    e2_d = out["metric"].apply(out["embeddings"])
    unit = torch.from_numpy(stage.state()["rows"]).cuda()[None]
    assert same_bits(H.holdout_logits(e2_d, unit, np.zeros(m, dtype=np.int32)).cpu().numpy(), logits.cpu().numpy())
    sc = H.score_plans(e2_d, exp, ids, np.zeros(m, dtype=np.int32), rows, [dict(train=0, eval=1, mix=1.0, min_windows=1)], vote=9,
                       return_sequences=True)
    assert torch.equal(sc["pred"][0], pred) and torch.equal(sc["voted"][0], voted)
    assert int(sc["voted_hit"][0]) == int((want["voted"][exp >= 0] == exp[exp >= 0]).sum())
    # the logits go through the gate sweep as any decoder's logits do
    configs = [dict(min_votes=1), dict(min_votes=3, dwell=2, min_margin=0.01), dict(min_cosine=0.2, weight="margin")]
    a, b = sweep_gate(logits, exp, ids, configs), sweep_gate(torch.from_numpy(want["logits"]).cuda(), exp, ids, configs)
    assert all(np.array_equal(a[key], b[key]) for key in b) and len(b) >= 10
    # a gate stacked on the stage: with every gate open its command is the stage's vote
    stage.reset()
    gate = CommandGate(stage)
    g_pred, g_voted, g_logits, command, accepted, conf, margin = gate.push(raw[:5000], return_logits=True)
    n = g_pred.shape[0]
    assert torch.equal(g_pred, pred[:n]) and torch.equal(g_voted, voted[:n]) and torch.equal(command, g_voted)
    assert same_floats(g_logits.cpu().numpy(), want["logits"][:n]) and g_logits.shape[1] == 4
    # a drive stacked on the stage follows its vote: it equals the drive alone on what the stage returned
    stage.reset()
    s_pred, s_voted, s_wins = stage.push(raw[:5000], return_windows=True)
    assert torch.equal(s_voted, voted[:n]) and s_wins.shape == (n, 12)
    profile = drive_profile(s_wins, exp[:n], ids, min_windows=10)
    alone = GraspDrive(stage, profile=profile, smooth=5).apply(s_wins, s_voted)
    stage.reset()
    drive = GraspDrive(stage, profile=profile, smooth=5)
    assert drive.follow == "voted" and not drive.multi
    res = drive.push(raw[:5000])
    assert len(res) == 5 and torch.equal(res[1], s_voted) and all(torch.equal(x, y) for x, y in zip(res[2:], alone))
