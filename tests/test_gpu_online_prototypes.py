"""Posture prototypes on the MI355X (contrastiveprosthetics_amd/prototypes.py fit_prototypes, Prototypes.install and PostureRows,
csrc/online_prototypes.cuh) against the numpy definitions `fit_reference` and `group_reference`: the fit in every bit and
integer, the fit against shipped enrolment, the stage in every integer and bit, cut and neighbour invariance, singleton groups
behind the four decoders, and the chain from a recording to the gate.  Every comparison is exact; the payload bits of a NaN are
the one thing not compared (the definition does not set them)."""
import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import prototypes as P
from contrastiveprosthetics_amd._lib import CpNativeError
from test_gpu_online_track import KINDS, _recordings, chunks_of, engine, make_decoder, norm, same_floats  # noqa: F401 (fixtures)
from test_online_prototypes_host import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
R, I = P.REST, P.IGNORE


# ---------------------------------------------------------------------------------------------------------------------------
# the fit against the definition
# ---------------------------------------------------------------------------------------------------------------------------
def fit_case(m, k, seed):
    """a recording of m windows over k class ids that has what the fit must get right: clusters, duplicate windows, IGNORE
    and REST windows, a class that is absent, one with a handful of windows, a NaN, an Inf and an all-zero window (only
    in the short recordings: no window is farther from every centre, so it takes every farthest-first round)"""
    rng = np.random.default_rng(seed)
    ids = np.arange(k) * 3 + 2
    centres = rng.standard_normal((k, 3, 16))
    present = np.arange(k) if k < 3 else np.delete(np.arange(k), k // 2)       # class k // 2 never appears
    slot = rng.choice(present, size=m)
    if k >= 3 and m >= 64:
        rare = present[-1]
        slot[slot == rare] = present[0]
        slot[rng.choice(m, size=3, replace=False)] = rare                      # three windows: fewer than rows, or than min_windows
    emb = centres[slot, rng.integers(0, 3, size=m)] + 0.4 * rng.standard_normal((m, 16))
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(F)
    exp = ids[slot].astype(np.int64)
    if m >= 15:
        emb[m // 2:m // 2 + 4] = emb[1]                        # duplicates: they tie in farthest-first and in the assignment
        exp[m // 2:m // 2 + 4] = exp[1]
        exp[3], exp[m - 2] = I, R
        emb[5, 7], emb[6, 0] = np.nan, np.inf
        if m < 700:
            emb[8] = 0.0
    if m >= 700:
        emb[rng.choice(m, size=40, replace=False), rng.integers(0, 16, size=40)] = np.nan
        exp[rng.choice(m, size=60, replace=False)] = rng.choice([R, I], size=60)
    return emb, exp, ids


def assert_fit(got: P.Prototypes, want: dict, what):
    for name in ("counts", "valid", "moved"):
        assert same_bits(getattr(got, name), want[name]), (what, name, getattr(got, name), want[name])
    a = got.assign.cpu().numpy()
    bad = np.nonzero(a != want["assign"])[0]
    assert a.dtype == np.int32 and bad.size == 0, (what, "assign", bad[:5], a[bad[:5]], want["assign"][bad[:5]])
    assert same_bits(got.rows.cpu().numpy(), want["rows"]), (what, "rows")


MIXED16 = [1, 2, 3, 4] * 4
FIT_CASES = [  # m, k, rows_per_class, iters, min_windows, use
    (1, 1, 1, 0, 1, False), (1, 2, 4, 10, 1, False), (15, 2, 2, 1, 1, False), (16, 1, 3, 10, 1, True), (17, 2, 4, 10, 2, False),
    (63, 2, 3, 10, 3, True), (64, 16, 2, 1, 1, False), (65, 16, MIXED16, 10, 2, True), (700, 1, 4, 10, 5, False),
    (700, 2, 1, 10, 25, True), (700, 16, 4, 10, 4, True), (700, 16, MIXED16, 0, 4, False), (700, 41, 1, 1, 4, False),
    (700, 41, [2] * 23 + [1] * 18, 10, 4, True), (700, 64, 1, 10, 4, True), (700, 16, 3, 1, 1, False),
]


@pytest.mark.parametrize("m,k,rows,iters,minw,masked", FIT_CASES)
def test_fit_equals_the_definition(m, k, rows, iters, minw, masked):
    emb, exp, ids = fit_case(m, k, seed=m + k)
    use = np.random.default_rng(m * k).random(m) < 0.8 if masked else None
    want = P.fit_reference(emb, exp, ids, rows, iters=iters, min_windows=minw, use=use)
    if m >= 700 and k <= 16:                                   # the input makes the fit work: counted on the definition
        assert want["valid"].any() and (iters == 0 or rows == 1 or (want["moved"][:, 1:] > 0).any() or iters == 1)
        assert (want["assign"] == -1).sum() >= 40
    got = P.fit_prototypes(torch.from_numpy(emb).cuda(), exp, ids, rows, iters=iters, min_windows=minw, use=use)
    assert_fit(got, want, (m, k, rows, iters, minw, masked))


def test_fit_input_covers_the_hard_cases_and_a_class_does_not_depend_on_the_others():
    emb, exp, ids = fit_case(700, 16, seed=9)
    want = P.fit_reference(emb, exp, ids, 4, iters=10, min_windows=4)
    fitted = want["valid"].any(axis=1)
    assert not fitted[8] and want["counts"][8].sum() == 0                      # absent
    assert not fitted[15] and (want["assign"][exp == ids[15]] == -1).all()     # three windows < min_windows
    assert (~want["valid"][fitted]).any()                                      # a centre below min_windows is dropped
    assert want["assign"][[5, 6]].tolist() == [-1, -1] and (want["moved"][:, 1] > 0).any()
    few = P.fit_reference(emb, exp, ids, 4, iters=3, min_windows=1)            # three windows, four rows
    assert few["valid"][15].sum() <= 3 and few["counts"][15].sum() == 3
    dev = torch.from_numpy(emb).cuda()
    assert_fit(P.fit_prototypes(dev, exp, ids, 4, iters=3, min_windows=1), few, "fewer windows than rows")
    full = P.fit_prototypes(dev, exp, ids, 4, iters=10, min_windows=4)
    assert_fit(full, want, "full")
    zemb = emb.copy()                                          # an all-zero window is finite: it trains, and is a centre
    z = int(np.nonzero((exp == ids[0]) & np.isfinite(emb).all(axis=1))[0][0])
    zemb[z] = 0.0
    zwant = P.fit_reference(zemb, exp, ids, 4, iters=10, min_windows=4)
    assert zwant["assign"][z] >= 0 and not zwant["rows"][0, 1].any() and zwant["valid"][0, 0]
    assert_fit(P.fit_prototypes(torch.from_numpy(zemb).cuda(), exp, ids, 4, iters=10, min_windows=4), zwant, "a zero window")
    for c in (0, 3, 15):
        alone = P.fit_prototypes(dev, np.where(exp == ids[c], exp, R), ids[c:c + 1], 4, iters=10, min_windows=4)
        assert same_bits(alone.rows.cpu().numpy()[0], want["rows"][c]) and same_bits(alone.counts[0], want["counts"][c])
        assert same_bits(alone.moved[0], want["moved"][c]) and same_bits(alone.valid[0], want["valid"][c])
        sel = exp == ids[c]
        assert same_bits(alone.assign.cpu().numpy()[sel], want["assign"][sel])
    with pytest.raises(ValueError, match="rows_per_class"):
        P.fit_prototypes(dev, exp, ids, 5)


def test_one_row_per_class_is_shipped_enrolment_with_a_zero_prior(engine, norm):
    from contrastiveprosthetics_amd.online import OnlineDecoder, window_labels
    from contrastiveprosthetics_amd.track import embed_recording
    mean, std = norm
    raw = _recordings(1, seed=41, length=6200)[0]
    ids = np.array([3, 8, 20])
    rng = np.random.default_rng(4)
    labels = np.repeat(ids[rng.integers(0, 3, size=62)], 100).astype(np.int64)
    labels[np.repeat(rng.random(62) < 0.3, 100)] = -1                          # masked: these samples enrol nothing
    dec = OnlineDecoder(engine, mean, std, vote=9, dtype="f32")
    dec.set_classes(table=torch.zeros(3, 16), ids=ids)                         # prior rows of zero
    dec.enroll(raw, labels, mix=1.0, min_windows=5)
    table, got_ids = dec.class_table()
    wl = window_labels(labels, 0)
    fit = P.fit_prototypes(embed_recording(dec, raw), np.where(wl >= 0, wl, R), ids, 1, iters=10, min_windows=5)
    assert got_ids.tolist() == ids.tolist() and fit.valid[:, 0].all()
    assert same_bits(fit.rows.cpu().numpy()[:, 0], table.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# the stage against the definition
# ---------------------------------------------------------------------------------------------------------------------------
class Source:
    """the part of a decoder that PostureRows.apply reads: the row ids, a sample count and a vote length"""
    device = torch.device("cuda:0")
    ws = None

    def __init__(self, ids, vote, multi=False):
        cid = [None if i is None else torch.as_tensor(np.asarray(i), dtype=torch.int32) for i in (ids if multi else [ids])]
        self.class_ids = cid if multi else cid[0]
        self.vote = vote
        self.n_seen = np.zeros(len(cid), dtype=np.int64) if multi else 0

    def push(self, *a, **k):
        raise AssertionError("apply() does not push the decoder")


def stage_case(n, rows, groups, seed):
    """row logits (n, rows) with ties, signed zeros and rows that are not finite; ascending row ids; one class id per row"""
    rng = np.random.default_rng(seed)
    rid = np.sort(rng.choice(400, size=rows, replace=False))
    gids = np.sort(rng.choice(90, size=groups, replace=False))
    cls = np.concatenate([gids, rng.choice(gids, size=rows - groups)])[rng.permutation(rows)]
    l = (rng.standard_normal((n, rows)) * 0.3).astype(F)
    l = np.round(l * 8) / 8 if seed % 2 else l                 # coarse values: many ties within and across groups
    l = l.astype(F)
    l[l == 0] = np.where(rng.random((l == 0).sum()) < 0.5, F(-0.0), F(0.0))
    for j, v in zip(rng.choice(n, size=min(12, n // 8), replace=False), [np.nan, np.inf, -np.inf] * 4):
        l[j, rng.integers(0, rows)] = v
    return l, rid, cls


def apply_cuts(stage, l, cuts):
    dev = torch.from_numpy(l).cuda()
    outs, p = [], 0
    for n in cuts:
        outs.append(stage.apply(dev[p:p + n]))
        p += n
    assert p == l.shape[0]
    return [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(4)]


def assert_stage(got, want, what):
    pred, voted, row, logits = got
    for name, g in (("pred", pred), ("voted", voted), ("row", row)):
        bad = np.nonzero(g.astype(np.int64) != want[name])[0]
        assert g.dtype == np.int32 and bad.size == 0, (what, name, bad[:5], g[bad[:5]], want[name][bad[:5]])
    assert same_floats(logits, want["logits"]), (what, "logits")


@pytest.mark.parametrize("windows", [1, 25, 256])
@pytest.mark.parametrize("vote", [1, 25, 256])
@pytest.mark.parametrize("rows,groups", [(1, 1), (2, 1), (2, 2), (63, 41), (64, 16), (64, 64)])
def test_stage_equals_the_definition(rows, groups, vote, windows):
    n = 600 if windows > 1 else 90
    l, rid, cls = stage_case(n, rows, groups, seed=rows + groups + vote)
    want = P.group_reference(l, rid, cls, vote=vote)
    assert (want["pred"] == -1).sum() >= 6 and want["ids"].shape[0] == groups
    assert rows == 1 or len(set(want["row"].tolist())) > 2
    stage = P.PostureRows(Source(rid, vote), cls)
    cuts = [windows] * (n // windows) + ([n % windows] if n % windows else [])
    assert_stage(apply_cuts(stage, l, cuts), want, (rows, groups, vote, windows))
    assert stage.class_ids.tolist() == want["ids"].tolist()
    st = stage.state()
    assert st["row_ids"] == rid.tolist() and st["class_ids"] == want["ids"].tolist() and len(st["ring"]) == min(vote, n)
    assert [want["ids"][g] for g in st["group_of"]] == cls.tolist()


def test_any_cut_gives_the_same_outputs():
    l, rid, cls = stage_case(1020, 40, 13, seed=3)
    want = P.group_reference(l, rid, cls, vote=25)
    for cut in (1020, 1, 7, 64, 255):
        stage = P.PostureRows(Source(rid, 25), cls)
        got = apply_cuts(stage, l, [cut] * (1020 // cut) + ([1020 % cut] if 1020 % cut else []))
        assert_stage(got, want, cut)


def test_three_streams_with_their_own_groupings_share_a_launch_and_idle_streams_stay():
    cases = [stage_case(300, 64, 16, seed=1), stage_case(300, 7, 7, seed=2), stage_case(300, 30, 4, seed=3)]
    ids = [c[1] for c in cases] + [None, cases[0][1]]          # stream 3 has no groups, stream 4 never gets windows
    maps = [c[2] for c in cases] + [None, cases[0][2]]
    stage = P.PostureRows(Source(ids, 25, multi=True), maps)
    dev = [torch.from_numpy(c[0]).cuda() for c in cases]
    outs, p = [], 0
    for n in (1, 64, 200, 35):                                 # stream 1 sits the second launch out
        sit = n == 64
        before = stage.state(1) if sit else None
        outs.append(stage.apply([dev[0][p:p + n], None if sit else dev[1][p:p + n], dev[2][p:p + n], None, None]))
        if sit:
            assert stage.state(1) == before and outs[-1][1][0].shape == (0,)
        assert outs[-1][3][0].shape == (0,) and outs[-1][4][3].shape == (0, 16)
        p += n
    assert stage.state(3) == dict(row_ids=[], group_of=[], class_ids=[], ring=[]) and stage.state(4)["ring"] == []
    for s, (l, rid, cls) in enumerate(cases):
        if s == 1:                                             # its own windows, in its own order
            l = np.concatenate([l[:1], l[65:300]])
        want = P.group_reference(l, rid, cls, vote=25)
        got = [torch.cat([o[s][i] for o in outs]).cpu().numpy() for i in range(4)]
        assert_stage(got, want, s)
        alone = P.PostureRows(Source(rid, 25), cls)
        assert_stage(apply_cuts(alone, l, [l.shape[0]]), want, (s, "alone"))
    with pytest.raises(CpNativeError, match="no class list"):
        stage.apply([None, None, None, dev[0][:3], None])
    with pytest.raises(ValueError, match="columns"):
        stage.apply([dev[1][:3], None, None, None, None])


def test_streams_of_a_multi_stream_decoder_with_their_own_installs_equal_their_single_stream_runs(engine, norm):
    """a plain neighbour, a stream with an install, one with an install through stage= that needs a fallback row, and one
    without classes, in one MultiStreamDecoder: each stream's outputs equal those of an OnlineDecoder with the same table and
    its own stage"""
    from contrastiveprosthetics_amd.online import MultiStreamDecoder, OnlineDecoder, windows_before
    from contrastiveprosthetics_amd.track import embed_recording
    mean, std = norm
    recs = _recordings(3, seed=61, length=6200)
    m = windows_before(6200, 0)
    dec = MultiStreamDecoder(engine, mean, std, 4, vote=9, dtype="f32")
    dec.set_classes(0, classes=list(range(41)))                # the neighbour keeps one row per class
    dec.set_classes(2, classes=[0, 1, 2, 5, 7])
    fits = {}
    for s, (k, rows, seed) in ((1, (3, [2, 3, 1], 1)), (2, (4, 2, 2))):
        _, exp, _ = P.posture_recording(m, k, 2, seed=seed, segment=30, rest=8)
        if s == 1:
            dec.set_classes(1, classes=[9])                    # (embedding needs a table; it is replaced by the install)
        ids = np.arange(k) if s == 1 else np.array([0, 1, 2, 5, 7])            # classes 5 and 7 have no window: not fitted
        exp = np.where(exp == 3, R, exp)
        fits[s] = P.fit_prototypes(embed_recording(dec, recs[s], s), exp, ids, rows, iters=5, min_windows=10)
    assert fits[1].fitted.all() and fits[2].fitted.tolist() == [True, True, True, False, False]
    prior2 = dec.class_table(2)[0].cpu().numpy()
    stage = fits[1].install(dec, 1)
    assert stage.class_ids[0].tolist() == list(range(41)) and stage.class_ids[1].tolist() == [0, 1, 2]     # the neighbour: singletons
    assert stage.class_ids[2].tolist() == [0, 1, 2, 5, 7] and stage.class_ids[3] is None
    assert fits[2].install(dec, 2, stage=stage) is stage
    table2, rid2 = (x.cpu().numpy() for x in dec.class_table(2))
    assert rid2[-2:].tolist() == [20, 28] and same_bits(table2[-2:], prior2[-2:]) and len(rid2) >= 5       # the current rows of 5 and 7
    assert stage.class_ids[2].tolist() == [0, 1, 2, 5, 7] and stage.row_ids(2).tolist() == rid2.tolist()
    fits[2].install(dec, 2, stage=stage)                       # again: the decoder's ids are row ids now, the stage maps them
    again, rid_again = (x.cpu().numpy() for x in dec.class_table(2))
    assert same_bits(again, table2) and rid_again.tolist() == rid2.tolist()
    with pytest.raises(ValueError, match="not fitted"):        # without the stage row ids 20 and 28 are not classes 5 and 7
        fits[2].install(dec, 2)
    assert same_bits(dec.class_table(2)[0].cpu().numpy(), table2)
    with pytest.raises(ValueError, match="stream"):
        fits[1].install(dec)
    with pytest.raises(IndexError):
        fits[1].install(dec, 4)
    # the single-stream twins
    maps = [None, P.class_of_row, P.class_of_row]
    twins = []
    for s in range(3):
        one = OnlineDecoder(engine, mean, std, vote=9, dtype="f32")
        t, i = dec.class_table(s)
        one.set_classes(table=t, ids=i.numpy())
        twins.append(P.PostureRows(one, maps[s]))
    dec.reset()
    stage.reset()
    pos = [0, 0, 0]
    for launch, ns in enumerate(((700, 21, 300), (1, 900, 0), (2500, 340, 1200), (40, 0, 4000))):
        chunks = [recs[s][pos[s]:pos[s] + n] if n else None for s, n in enumerate(ns)] + [None]
        if launch == 2:
            raw = torch.cat([c for c in chunks if c is not None])
            got = stage.push_packed(raw, list(ns) + [0], return_logits=True, return_rows=True)
        else:
            got = stage.push(chunks, return_logits=True, return_rows=True)
        assert len(got) == 4 and got[3][0].shape == (0,)
        for s, n in enumerate(ns):
            want = twins[s].push(recs[s][pos[s]:pos[s] + n], return_logits=True, return_rows=True) if n else None
            pos[s] += n
            if want is None:
                assert got[s][0].shape == (0,)
                continue
            for x, y, name in zip(got[s], want, ("pred", "voted", "logits", "row")):
                assert x.shape == y.shape and x.dtype == y.dtype and same_bits(x.cpu().numpy(), y.cpu().numpy()), (launch, s, name)
    # a grouping changed on one stream alone
    stage.set_class_of_row(0, lambda r: r // 8)
    assert stage.class_ids[0].tolist() == list(range(6)) and stage.class_ids[1].tolist() == [0, 1, 2]
    out = stage.push([recs[0][:400], None, None, None], return_rows=True)
    assert len(out[0]) == 3 and torch.equal(out[0][0], out[0][2] // 8)
    with pytest.raises(TypeError):
        stage.set_class_of_row(None)


@pytest.mark.parametrize("kind", KINDS)
def test_singleton_groups_behind_a_decoder_are_the_decoder(engine, norm, kind):
    recs = _recordings(2, seed=31)
    staged, plain = make_decoder(kind, engine, norm, "f32"), make_decoder(kind, engine, norm, "f32")
    stage = P.PostureRows(staged, None)
    multi = kind.startswith("multi")
    rng = np.random.default_rng(2)
    p = 0
    while p < 3000:
        n = int(rng.integers(1, 900))
        a = stage.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True, return_rows=True)
        b = plain.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True)
        p += n
        for s, (ra, rb) in enumerate(zip(a, b) if multi else [(a, b)]):
            assert len(ra) == 5
            for x, y, name in zip(ra, rb, ("pred", "voted", "logits", "windows")):
                assert x.shape == y.shape and x.dtype == y.dtype and same_bits(x.cpu().numpy(), y.cpu().numpy()), (kind, p, s, name)
            assert torch.equal(ra[4], ra[0])                   # every row is its own class
    ids = stage.class_ids
    assert (ids[0] if multi else ids).tolist() == sorted((plain.class_ids[0] if multi else plain.class_ids).tolist())
    if multi:
        raw = torch.cat([recs[0][:400], recs[1][:100]])
        for d in (stage, plain):
            d.reset()
        a, b = stage.push_packed(raw, [400, 100, 0, 0], return_logits=True), plain.push_packed(raw, [400, 100, 0, 0], return_logits=True)
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) for x, y in zip(a, b))
    else:
        with pytest.raises(TypeError):
            stage.push_packed(recs[0][:40], [40])
    # a push of the decoder behind the stage's back is refused before anything is enqueued
    staged.push(chunks_of(kind, recs, 0, 40))
    with pytest.raises(CpNativeError, match="behind the posture stage"):
        stage.push(chunks_of(kind, recs, 40, 40))
    stage.reset()
    stage.push(chunks_of(kind, recs, 0, 40))


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: a recording, the fit, the install, the stage, the sweeps and the gate
# ---------------------------------------------------------------------------------------------------------------------------
def test_from_a_recording_to_class_commands(engine, norm):
    from contrastiveprosthetics_amd.online import CommandGate, OnlineDecoder, sweep_gate, sweep_subsets, windows_before
    from contrastiveprosthetics_amd.track import embed_recording
    mean, std = norm
    raw = _recordings(1, seed=51, length=12400)[0]
    m = windows_before(raw.shape[0], 0)
    _, exp, _ = P.posture_recording(m, 4, 2, seed=0, segment=30, rest=8)       # the cue schedule of the posture recording
    ids = np.array([0, 1, 2, 3])
    rep, n_rep = H.repetitions(exp)
    use = rep < n_rep - 2
    dec = OnlineDecoder(engine, mean, std, classes=[0, 1, 2, 3, 7], vote=9, dtype="f32")
    emb = embed_recording(dec, raw)
    assert emb.shape == (m, 16)
    fit = P.fit_prototypes(emb, exp, ids, [2, 1, 3, 2], iters=10, min_windows=10, use=use)
    assert_fit(fit, P.fit_reference(emb.cpu().numpy(), exp, ids, [2, 1, 3, 2], iters=10, min_windows=10, use=use), "end to end")
    assert fit.fitted.all() and fit.valid.sum() > 4
    stage = fit.install(dec)
    table, rid = fit.table()
    assert dec.class_ids.tolist() == rid.tolist() and stage.class_ids.tolist() == ids.tolist()
    assert stage.row_ids().tolist() == rid.tolist() and P.class_of_row(int(rid[-1])) == 3
    twin = OnlineDecoder(engine, mean, std, vote=9, dtype="f32")
    twin.set_classes(table=torch.from_numpy(table), ids=rid)
    outs, rows_l, p = [], [], 0
    for n in (4000, 37, 2600, 5763):
        outs.append(stage.push(raw[p:p + n], return_logits=True, return_rows=True))
        rows_l.append(twin.push(raw[p:p + n], return_logits=True)[2])
        p += n
    pred, voted, logits, row = (torch.cat([o[i] for o in outs]) for i in range(4))
    row_logits = torch.cat(rows_l).cpu().numpy()
    want = P.group_reference(row_logits, rid, vote=9)
    assert_stage([pred.cpu().numpy(), voted.cpu().numpy(), row.cpu().numpy(), logits.cpu().numpy()], want, "end to end")
    held = torch.from_numpy(np.nonzero(~use)[0]).cuda()
    assert len(set(row.cpu().numpy()[~use].tolist())) > 2
    # the class logits go through the sweeps as any decoder's logits do
    configs = [dict(min_votes=1), dict(min_votes=3, dwell=2, min_margin=0.01), dict(min_cosine=0.2, weight="margin")]
    ref_logits = torch.from_numpy(want["logits"]).cuda()
    a, b = sweep_gate(logits[held], exp[~use], ids, configs), sweep_gate(ref_logits[held], exp[~use], ids, configs)
    assert all(np.array_equal(a[key], b[key]) for key in b) and len(b) >= 10
    subsets = [[0, 1], [0, 1, 2, 3], [1, 3]]
    a, b = sweep_subsets(logits[held], exp[~use], ids, subsets, vote=9), sweep_subsets(ref_logits[held], exp[~use], ids, subsets, vote=9)
    assert all(np.array_equal(a[key], b[key]) for key in b)
    # a gate stacked on the stage: with every gate open its command is the stage's vote
    stage.reset()
    gate = CommandGate(stage)
    g_pred, g_voted, g_logits, command, accepted, conf, margin = gate.push(raw[:5000], return_logits=True)
    n = g_pred.shape[0]
    assert torch.equal(g_pred, pred[:n]) and torch.equal(g_voted, voted[:n]) and torch.equal(command, g_voted)
    assert same_floats(g_logits.cpu().numpy(), want["logits"][:n]) and g_logits.shape[1] == 4
    # a drive stacked on the stage follows the class vote, on the gate on the stage the command: the windows and class ids it
    # reads are the stage's, so it equals the drive alone on what the stage returned
    from contrastiveprosthetics_amd.online import GraspDrive, drive_profile
    stage.reset()
    s_pred, s_voted, s_wins = stage.push(raw[:5000], return_windows=True)
    assert torch.equal(s_voted, voted[:n]) and s_wins.shape == (n, 12)
    profile = drive_profile(s_wins, exp[:n], ids, min_windows=10)
    alone = GraspDrive(stage, profile=profile, smooth=5).apply(s_wins, s_voted)
    stage.reset()
    drive = GraspDrive(stage, profile=profile, smooth=5)
    assert drive.follow == "voted" and not drive.multi
    out = drive.push(raw[:5000])
    assert len(out) == 5 and torch.equal(out[1], s_voted)
    assert all(torch.equal(x, y) for x, y in zip(out[2:], alone))
    stage.reset()
    both = GraspDrive(CommandGate(stage), profile=profile, smooth=5)
    assert both.follow == "command"
    out = both.push(raw[:5000])
    assert len(out) == 9 and torch.equal(out[2], s_voted) and all(torch.equal(x, y) for x, y in zip(out[6:], alone))
    # a new table on the decoder: the stage derives its groups again before the next launch
    dec.set_classes(classes=[0, 1, 2, 3, 7])
    stage.set_class_of_row(None)
    stage.reset()
    assert stage.class_ids.tolist() == [0, 1, 2, 3, 7]
    out = stage.push(raw[:400], return_rows=True)
    assert torch.equal(out[0], out[2])
