"""Held-out enrolment scoring on the MI355X (contrastiveprosthetics_amd/holdout.py score_plans, holdout_logits and
score_enrolment, csrc/online_holdout.cuh) against the numpy definition `holdout_reference`: every score, confusion cell,
sequence entry and bit of rows, unit rows, sums and logits; the order of the float64 sums; the shipped path (masked `enroll`, a
fresh decoder and a push); the four decoders; the chain into the gate and subset sweeps.  Every comparison is exact; the
payload bits of a NaN are the one thing not compared (the definition does not set them)."""
import ctypes

import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import holdout as H
from test_online_holdout_host import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
R, I = H.REST, H.IGNORE
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)


def same_floats(got, want):
    """bit-equal where `want` is a number, NaN where it is NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    iview = np.int32 if got.dtype == F else np.int64
    return bool(np.isnan(got[nan]).all() and (got.view(iview)[~nan] == want.view(iview)[~nan]).all())


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


# ---------------------------------------------------------------------------------------------------------------------------
# synthetic embeddings straight into the entries
# ---------------------------------------------------------------------------------------------------------------------------
def recording(m, k, reps, seed, bad_rows=True):
    """m windows of k classes (ids that are not their slots) in segments of 1..7 windows, some followed by rest and some not, some
    IGNORE windows, class 0 absent from the last fold, a few windows without a repetition and a few that are not numbers"""
    rng = np.random.default_rng(seed)
    ids = np.arange(k) * 2 + 1
    centre = rng.standard_normal((k, 16))
    exp = np.zeros(m, dtype=np.int64)
    i, c = 0, 0
    while i < m:
        n = int(rng.integers(1, 8))
        exp[i:i + n] = ids[c % k]
        i += n
        c += 1
        if rng.random() < 0.6:                                         # (else: a cue with no rest behind it)
            n = int(rng.integers(1, 5))
            exp[i:i + n] = R
            i += n
    exp[rng.random(m) < 0.05] = I
    rep, n_rep = H.repetitions(exp, folds=reps)
    if k > 1 and n_rep > 1:
        exp[(rep == n_rep - 1) & (exp == ids[0])] = R                  # a class that one fold does not have
        rep, n_rep = H.repetitions(exp, folds=reps)
    rep = rep.copy()
    if m > 20:
        rep[rng.random(m) < 0.04] = -1
    emb = centre[np.searchsorted(ids, np.maximum(exp, ids[0]))] + 0.8 * rng.standard_normal((m, 16))
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(F)
    if bad_rows and m > 60:
        emb[7, 3], emb[40, 0], emb[41] = np.nan, np.inf, 0.0
    prior = centre + 0.5 * rng.standard_normal((k, 16))
    prior = (prior / np.linalg.norm(prior, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (k, 1))).astype(F)
    return emb, exp, ids, rep, max(n_rep, 1), prior


def some_plans(n_rep, t, seed):
    """t plans: leave-one-out and the learning curve first, then random masks, mixes and min_windows, a refused plan among them"""
    rng = np.random.default_rng(seed)
    plans = H.leave_one_out(n_rep, mix=1.0, min_windows=2) + H.learning_curve(n_rep, mix=0.5, min_windows=1)
    plans = plans[:t]
    while len(plans) < t:
        plans.append(dict(train=int(rng.integers(0, 2 ** n_rep)), eval=int(rng.integers(0, 2 ** n_rep)),
                          mix=float(rng.choice([0.0, 0.25, 1.0, rng.random()])), min_windows=int(rng.choice([1, 2, 5, 25]))))
    if t > 4:
        plans[3] = dict(plans[3], mix=1.5)
        plans[-1] = dict(plans[-1], min_windows=0)
    return plans


def assert_equals_definition(emb, exp, ids, rep, prior, plans, vote):
    ref = H.holdout_reference(emb, exp, ids, rep, prior, plans, vote=vote, return_sequences=True)
    emb_d = torch.from_numpy(emb).cuda()
    got = H.score_plans(emb_d, exp, ids, rep, prior, plans, vote=vote, confusion=True, return_sequences=True)
    for key in H.HOLDOUT_SCORE_KEYS:
        assert got[key].dtype == np.int64 and np.array_equal(got[key], ref[key]), (key, got[key], ref[key])
    k = len(ids)
    assert same_floats(host(got["rows"]), ref["rows"]) and same_floats(host(got["unit"]), ref["unit"])
    sums = host(got["sums"])
    assert sums.shape[1:] == (64, 17) and not sums[:, k:].any()
    for t in np.nonzero(ref["n_cue"] >= 0)[0]:
        u = got["sums_index"][t]
        assert same_floats(sums[u, :k, :16], ref["sums"][t]) and np.array_equal(sums[u, :k, 16], ref["counts"][t].astype(np.float64)), t
    assert np.array_equal(host(got["confusion"]), ref["confusion"]) and np.array_equal(host(got["voted_confusion"]), ref["voted_confusion"])
    assert np.array_equal(host(got["pred"]), ref["pred"]) and np.array_equal(host(got["voted"]), ref["voted"])
    plain = H.score_plans(emb_d, exp, ids, rep, prior, plans, vote=vote)           # the kernel without the confusion tables
    assert all(np.array_equal(plain[key], ref[key]) for key in H.HOLDOUT_SCORE_KEYS) and "confusion" not in plain and "pred" not in plain
    for most in (False, True):
        assign = H.assign_folds(rep, plans, most_trained=most)
        logits = H.holdout_logits(emb_d, got, assign)
        assert same_floats(host(logits), H.holdout_logits_reference(emb, ref["unit"], assign))
    return ref, got


# M, K, R, T, vote: every M at a tile edge, every K, R and T the issue names, the three ring lengths
CASES = [(1, 1, 1, 1, 1), (15, 2, 2, 2, 25), (16, 41, 2, 65, 1), (17, 64, 6, 2, 25), (63, 2, 6, 65, 256), (64, 41, 6, 1, 25),
         (65, 2, 6, 4096, 25), (65, 64, 32, 65, 1), (700, 41, 6, 65, 25), (700, 2, 32, 65, 256), (700, 64, 6, 2, 1), (700, 1, 2, 65, 25)]


@pytest.mark.parametrize("m,k,reps,t,vote", CASES)
def test_device_equals_the_definition(m, k, reps, t, vote):
    emb, exp, ids, rep, n_rep, prior = recording(m, k, reps, seed=m + k + reps)
    if (m, reps) == (700, 32):
        assert n_rep == 32
    ref, _ = assert_equals_definition(emb, exp, ids, rep, prior, some_plans(n_rep, t, seed=t), vote)
    if m == 700:
        assert (ref["n_cue"] > 0).any() and (ref["pred_hit"] > 0).any() and (rep < 0).any() and (exp == I).any()
        assert (ref["pred"] == -1).any()                                           # the rows that are not numbers


def test_a_plans_results_do_not_depend_on_the_other_plans():
    emb, exp, ids, rep, n_rep, prior = recording(700, 41, 6, seed=5)
    plans = some_plans(n_rep, 65, seed=9)
    emb_d = torch.from_numpy(emb).cuda()
    full = H.score_plans(emb_d, exp, ids, rep, prior, plans, vote=25, confusion=True, return_sequences=True)
    for t in (0, 3, 17, 40, 64):
        one = H.score_plans(emb_d, exp, ids, rep, prior, [plans[t]], vote=25, confusion=True, return_sequences=True)
        for key in H.HOLDOUT_SCORE_KEYS:
            assert one[key][0] == full[key][t], (t, key)
        for key in ("rows", "unit", "confusion", "voted_confusion", "pred", "voted"):
            assert same_floats(host(one[key][0]), host(full[key][t])) if key in ("rows", "unit") else \
                np.array_equal(host(one[key][0]), host(full[key][t])), (t, key)


def test_the_sums_follow_window_order():
    """Unit embeddings do not show the order of a float64 sum, so the components are spread over 45 binary orders of magnitude;
    that the order matters at that spread is asserted on these inputs first"""
    rng = np.random.default_rng(4)
    k, m = 3, 1200
    emb, exp, ids, rep, n_rep, prior = recording(m, k, 6, seed=8, bad_rows=False)
    emb = (rng.standard_normal((m, 16)) * np.exp2(-rng.integers(0, 46, (m, 16)).astype(np.float64))).astype(F)
    plans = H.leave_one_out(n_rep, mix=1.0, min_windows=1) + [dict(train=2 ** n_rep - 1, eval=1, mix=1.0, min_windows=1)]
    slots = np.where(exp >= 0, np.searchsorted(ids, np.maximum(exp, 0)), exp)
    reversed_differs = segments_differ = 0
    for p in plans:
        for c in range(k):
            sel = np.nonzero((slots == c) & (rep >= 0) & ((p["train"] >> np.maximum(rep, 0)) & 1 == 1))[0]
            assert sel.size > 100
            x = emb[sel].astype(np.float64)
            fwd = np.cumsum(x, axis=0)[-1]
            reversed_differs += int((fwd != np.cumsum(x[::-1], axis=0)[-1]).sum())
            cuts = np.nonzero(np.diff(sel) > 1)[0] + 1
            parts = [np.cumsum(s, axis=0)[-1] for s in np.split(x, cuts)]
            segments_differ += int((fwd != np.cumsum(np.array(parts), axis=0)[-1]).sum())
    assert reversed_differs > 0 and segments_differ > 0
    assert_equals_definition(emb, exp, ids, rep, prior, plans, 25)


def test_slots_repetitions_plans_and_assignments_out_of_range_on_the_device_are_not_indexed_with():
    """the C entries take device arrays the host cannot check: a slot >= K or < -1 is a window that trains nothing and is not
    scored, a repetition outside 0..31 one that is neither trained nor evaluated, a bad plan scores -1, a bad assignment is NaN"""
    from contrastiveprosthetics_amd import _lib
    lib = _lib.load()
    emb, exp, ids, rep, n_rep, prior = recording(300, 5, 4, seed=3, bad_rows=False)
    k, m = 5, 300
    slots = np.where(exp >= 0, np.searchsorted(ids, np.maximum(exp, 0)), exp).astype(np.int32)
    rng = np.random.default_rng(0)
    wild_slot, wild_rep = slots.copy(), rep.astype(np.int32).copy()
    at = rng.choice(m, 40, replace=False)
    wild_slot[at[:20]] = [5, 63, 64, 1000, 2 ** 31 - 1, -3, -1000, -2 ** 31, 7, 6] * 2
    wild_rep[at[20:]] = [32, 33, 64, 2 ** 31 - 1, -2, -2 ** 31, 1000, 40, 32, -7] * 2
    clean_exp, clean_rep = exp.copy(), rep.copy()
    clean_exp[at[:20]] = I
    clean_rep[at[20:]] = -1
    plans = H.leave_one_out(n_rep, mix=0.5, min_windows=2)
    ref = H.holdout_reference(emb, clean_exp, ids, clean_rep, prior, plans, vote=9, return_sequences=True)
    table = np.zeros(len(plans) + 4, dtype=H._PLAN_DTYPE)
    masks = np.array([p["train"] for p in plans], dtype=np.uint32)
    for t, p in enumerate(plans):
        table[t] = (p["train"], p["eval"], t, 2, 0.5)
    table[-4] = (1, 1, len(plans), 2, 0.5)                             # a sums index one behind the last: no rows are made for it
    table[-3] = (1, 1, 4096, 2, 0.5)
    table[-2] = (1, 1, -1, 2, 0.5)
    table[-1] = (1, 1, 2 ** 31 - 1, 2, 0.5)
    n_plans, n_masks = len(table), len(masks)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    emb_d, slot_d, rep_d, prior_d = dev(emb), dev(wild_slot), dev(wild_rep), dev(prior)
    masks_d, plans_d = dev(masks.view(np.int32)), dev(table.view(np.uint8))
    sums = torch.full((n_masks, 64, 17), 7.0, dtype=torch.float64, device="cuda")
    rows, unit = (torch.zeros(n_plans, k, 16, device="cuda") for _ in range(2))
    scores = torch.zeros(n_plans, 9, dtype=torch.int64, device="cuda")
    conf, vconf = (torch.zeros(n_plans, 64, 64, dtype=torch.int32, device="cuda") for _ in range(2))
    pred, voted = (torch.full((n_plans, m), -3, dtype=torch.int32, device="cuda") for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.cp_online_holdout_sums(emb_d.data_ptr(), m, k, slot_d.data_ptr(), rep_d.data_ptr(), masks_d.data_ptr(), n_masks,
                                          sums.data_ptr(), stream), "sums")
    _lib.check(lib.cp_online_holdout_tables(sums.data_ptr(), n_masks, k, prior_d.data_ptr(), plans_d.data_ptr(), n_plans,
                                            rows.data_ptr(), unit.data_ptr(), stream), "tables")
    _lib.check(lib.cp_online_holdout_score(emb_d.data_ptr(), m, k, slot_d.data_ptr(), rep_d.data_ptr(), unit.data_ptr(),
                                           plans_d.data_ptr(), n_plans, 9, scores.data_ptr(), conf.data_ptr(), vconf.data_ptr(),
                                           pred.data_ptr(), voted.data_ptr(), stream), "score")
    assign = np.concatenate([H.assign_folds(clean_rep, plans)[:-6], [-1, -5, n_plans, n_plans + 1, 2 ** 31 - 1, -2 ** 31]]).astype(np.int32)
    logits = torch.zeros(m, k, device="cuda")
    _lib.check(lib.cp_online_holdout_logits(emb_d.data_ptr(), m, k, unit.data_ptr(), n_plans, dev(assign).data_ptr(), logits.data_ptr(), k,
                                            stream), "logits")
    n = len(plans)
    sc = scores.cpu().numpy()
    slot_of = {int(c): s for s, c in enumerate(ids)}
    for i, key in enumerate(H.HOLDOUT_SCORE_KEYS):
        want = ref[key] if key != "worst_class" else np.array([slot_of.get(int(c), -1) for c in ref[key]])
        assert np.array_equal(sc[:n, i], want), key
    assert not rows[n:].any() and not unit[n:].any()
    assert (sc[n + 1:] == -1).all() and (pred[n + 1:] == -3).all() and (voted[n + 1:] == -3).all() and not conf[n + 1:].any()
    s = sums.cpu().numpy()
    assert same_bits(s[:, :k, :16], ref["sums"]) and np.array_equal(s[:, :k, 16], ref["counts"]) and not s[:, k:].any()
    assert same_bits(host(rows[:n]), ref["rows"]) and same_bits(host(unit[:n]), ref["unit"])
    to_slot = np.vectorize(lambda c: slot_of.get(int(c), int(c)))
    assert np.array_equal(host(pred[:n]), to_slot(ref["pred"])) and np.array_equal(host(voted[:n]), to_slot(ref["voted"]))
    assert np.array_equal(host(conf[:n, :k, :k]), ref["confusion"]) and not conf[:, k:].any() and not conf[:, :, k:].any()
    assert np.array_equal(host(vconf[:n, :k, :k]), ref["voted_confusion"])
    want = H.holdout_logits_reference(emb, ref["unit"], np.where((assign >= 0) & (assign < n), assign, -1))
    assert same_floats(host(logits), want) and np.isnan(host(logits)[-6:]).all()


def test_wrappers_refuse_before_the_first_launch():
    emb, exp, ids, rep, n_rep, prior = recording(100, 3, 2, seed=1)
    emb_d = torch.from_numpy(emb).cuda()
    plans = H.leave_one_out(n_rep)
    for kw in (dict(vote=0), dict(vote=257), dict(plans=[]), dict(plans=[dict(train=1)]), dict(rep=rep[:-1]), dict(rep=rep + 31),
               dict(expected=np.where(exp >= 0, 4, exp)), dict(prior=np.zeros((3, 16), dtype=F)), dict(prior=prior[:2]), dict(ids=[3, 1, 5])):
        args = dict(embeddings=emb_d, expected=exp, ids=ids, rep=rep, prior=prior, plans=plans)
        args.update(kw)
        with pytest.raises(ValueError):
            H.score_plans(**args)
    with pytest.raises(ValueError):
        H.score_plans(emb_d[:0], exp[:0], ids, rep[:0], prior, plans)
    with pytest.raises(ValueError):
        H.holdout_logits(emb_d, torch.zeros(2, 3, 16), np.zeros(100, dtype=np.int32))      # unit rows on the host
    with pytest.raises(ValueError):
        H.holdout_logits(emb_d, torch.zeros(2, 3, 16, device="cuda"), np.zeros(99, dtype=np.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# against the shipped path, and behind the four decoders
# ---------------------------------------------------------------------------------------------------------------------------
CLASSES = [30, 2, 17, 5, 9]
IDS = np.array(sorted(CLASSES))
REST_LABEL = 0


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


@pytest.fixture(scope="module")
def cued():
    """5 classes x 3 repetitions of about 60 windows with rest between them: raw (n, 12) on the GPU, one label per sample (class
    id or REST_LABEL), the repetition of every sample, and the normalisation"""
    rng = np.random.default_rng(21)
    gains = 0.5 + 2.0 * rng.random((len(IDS), 12))
    raw, lab, srep = [], [], []
    for r in range(3):
        for c in rng.permutation(len(IDS)):
            n = int(rng.integers(1150, 1260))
            raw.append(rng.standard_normal((n, 12)) * gains[c] * 2e-3)
            lab.append(np.full(n, IDS[c]))
            srep.append(np.full(n, r))
            n = int(rng.integers(250, 400))
            raw.append(rng.standard_normal((n, 12)) * 4e-4)
            lab.append(np.full(n, REST_LABEL))
            srep.append(np.full(n, -1))
    raw = torch.from_numpy(np.concatenate(raw).astype(F)).cuda()
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    w = preprocess_segments(raw[None, :3000], keep=20 * np.arange(140))[0]
    return raw, np.concatenate(lab).astype(np.int64), np.concatenate(srep), (w.mean(0), w.std(0))


def make_decoder(kind, engine, norm, dtype, vote=9):
    from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, MultiStreamDecoder, OnlineDecoder
    mean, std = norm
    if kind == "single":
        return OnlineDecoder(engine, mean, std, classes=CLASSES, vote=vote, dtype=dtype), None
    if kind == "adapt":
        return OnlineDecoder(engine, mean, std, classes=CLASSES, vote=vote, dtype=dtype, adapt=0.0), None
    if kind == "multi":
        dec = MultiStreamDecoder(engine, mean, std, 3, vote=vote, dtype=dtype)
    else:
        dec = AdaptiveMultiStreamDecoder(engine, mean, std, 3, [0.01, 0.0, 0.02], vote=vote, dtype=dtype)
    dec.set_classes(0, classes=[7])
    dec.set_classes(1, classes=CLASSES)
    return dec, 1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_leave_one_out_equals_masked_enroll_a_fresh_decoder_and_a_push(engine, cued, dtype):
    from contrastiveprosthetics_amd.online import expected_commands
    from contrastiveprosthetics_amd.track import embed_recording
    raw, lab, srep, norm = cued
    dec, _ = make_decoder("single", engine, norm, dtype)
    exp = expected_commands(lab, IDS, rest=REST_LABEL)
    rep, n_rep = H.repetitions(exp)
    assert n_rep == 3 and (exp >= 0).sum() > 800 and (exp == R).sum() > 150
    prior = dec.class_table()[0]
    emb = embed_recording(dec, raw)
    mix, min_windows = 0.75, 25
    plans = H.leave_one_out(3, mix=mix, min_windows=min_windows) + [dict(train=0b111, eval=0b111, mix=mix, min_windows=min_windows)]
    got = H.score_plans(emb, exp, IDS, rep, prior, plans, vote=dec.vote, return_sequences=True)
    ref = H.holdout_reference(emb, exp, IDS, rep, prior, plans, vote=dec.vote, return_sequences=True)
    for key in H.HOLDOUT_SCORE_KEYS:
        assert np.array_equal(got[key], ref[key]), key
    assert same_bits(host(got["rows"]), ref["rows"]) and np.array_equal(host(got["pred"]), ref["pred"])
    assert (got["n_enrolled"] == 5).all() and (got["n_train"][:3] < got["n_train"][3]).all()
    for t, p in enumerate(plans):
        fresh, _ = make_decoder("single", engine, norm, dtype)
        held = (srep >= 0) & ((p["train"] >> np.maximum(srep, 0)) & 1 == 0)
        labels = np.where((lab == REST_LABEL) | held, -1, lab)
        counts = fresh.enroll(raw, labels, mix=mix, min_windows=min_windows)
        assert sum(counts.values()) == got["n_train"][t]
        assert same_bits(host(fresh.class_table()[0]), host(got["rows"][t])), t
        fresh.reset()
        pred, voted = (host(x) for x in fresh.push(raw))
        ev = host(got["pred"][t]) != H.NOT_EVALUATED
        assert ev.sum() > 300 and np.array_equal(pred[ev], host(got["pred"][t])[ev]), t
        if t == 3:
            assert ev.all() and np.array_equal(voted, host(got["voted"][t]))


@pytest.mark.parametrize("pair", [("single", "multi"), ("adapt", "multi_adapt")])
def test_score_enrolment_over_the_decoders_leaves_them_as_they_were(engine, cued, pair):
    from contrastiveprosthetics_amd.online import expected_commands, sweep_gate, sweep_subsets
    raw, lab, srep, norm = cued
    exp = expected_commands(lab, IDS, rest=REST_LABEL)
    results = []
    for kind in pair:
        dec, s = make_decoder(kind, engine, norm, "f32")
        if kind == "adapt":
            dec.calibrate(raw)
        elif kind == "multi_adapt":
            dec.calibrate(s, raw)
        warm = raw[:1234] if s is None else [raw[:700], raw[:1234], None]
        dec.push(warm)                                                          # a stream in mid-flight: ring, filter, count
        before, seen = dec.ws.clone(), np.array(dec.n_seen).copy()
        table = dec.class_table() if s is None else dec.class_table(s)
        out = H.score_enrolment(dec, raw, exp, plan="learning_curve", stream=s, mix=0.75, min_windows=25)
        after = dec.class_table() if s is None else dec.class_table(s)
        n_state = H._state_bytes(dec, s is not None)
        assert torch.equal(before[:n_state], dec.ws[:n_state]) and np.array_equal(seen, np.array(dec.n_seen))
        assert torch.equal(table[0], after[0]) and torch.equal(table[1], after[1])
        nxt = raw[1234:2468] if s is None else [None, raw[1234:2468], None]
        went_on = [host(x) for x in (dec.push(nxt) if s is None else dec.push(nxt)[s])]
        twin, _ = make_decoder(kind, engine, norm, "f32")                       # the same stream without the scoring in between
        if kind in ("adapt", "multi_adapt"):
            twin.calibrate(*(() if s is None else (s,)), raw)
        twin.push(warm)
        want = [host(x) for x in (twin.push(nxt) if s is None else twin.push(nxt)[s])]
        assert len(want[0]) > 50 and all(np.array_equal(x, y) for x, y in zip(went_on, want)) and torch.equal(twin.ws[:n_state], dec.ws[:n_state])
        results.append((out, went_on))
    (a, push_a), (b, push_b) = results
    assert all(np.array_equal(x, y) for x, y in zip(push_a, push_b))
    assert len(a["plans"]) == 6 and a["n_rep"] == 3 and sorted(a["curve"]) == [1, 2]
    for key in H.HOLDOUT_SCORE_KEYS:
        assert np.array_equal(a[key], b[key]), key
    for key in ("rows", "unit", "logits", "embeddings"):
        assert same_floats(host(a[key]), host(b[key])), key
    assert np.array_equal(a["assign"], b["assign"]) and np.array_equal(a["rep"], b["rep"]) and a["curve"] == b["curve"]
    # the definition on the same embeddings, and the curve from its counters
    emb = host(a["embeddings"])
    table = make_decoder(pair[0], engine, norm, "f32")[0].class_table()[0]
    ref = H.holdout_reference(emb, exp, IDS, a["rep"], table, a["plans"], vote=9)
    for key in H.HOLDOUT_SCORE_KEYS:
        assert np.array_equal(a[key], ref[key]), key
    assert same_bits(host(a["rows"]), ref["rows"])
    for n in (1, 2):
        of_n = [t for t, p in enumerate(a["plans"]) if bin(p["train"]).count("1") == n]
        assert a["curve"][n] == (int(ref["voted_hit"][of_n].sum()), int(ref["n_cue"][of_n].sum())) and a["curve"][n][1] == (exp >= 0).sum()
    assert np.array_equal(a["assign"], H.assign_folds(a["rep"], a["plans"], most_trained=True)) and (a["assign"] % 2 == 1).all()
    assert same_floats(host(a["logits"]), H.holdout_logits_reference(emb, ref["unit"], a["assign"]))
    # the held-out logits are what the sweeps take, as they are
    gate = sweep_gate(a["logits"], exp, IDS, [dict(min_votes=1), dict(min_votes=5, dwell=3)])
    assert gate["n_cue"][0] == (exp >= 0).sum()
    subsets = sweep_subsets(a["logits"], exp, IDS, [IDS.tolist(), IDS[:3].tolist()], vote=9)
    assert subsets["n_cue"][0] == (exp >= 0).sum() and 0 < subsets["voted_hit"][0] <= subsets["n_cue"][0]
