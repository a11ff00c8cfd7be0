"""Prototype tracking on the MI355X (contrastiveprosthetics_amd/track.py PrototypeTracker and sweep_tracker,
csrc/online_track.cuh) against the numpy definition `track_reference`: the embeddings a push gives out, the stage in every
integer and bit, cut and neighbour invariance, rate 0 behind the four decoders, adopt, the chain into the gate, and the sweep.
Every comparison is exact; the payload bits of a NaN are the one thing not compared (the definition does not set them)."""
import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import track as T
from contrastiveprosthetics_amd.track import PrototypeTracker, sweep_tracker, track_reference
from test_online_track_host import DRIFT, DRIFT_SETTINGS, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
OL_STATE, OL_TABLE = 7672, 3576          # one OlState per stream at the start of a decoder's workspace, and its unit rows


def same_floats(got, want):
    """bit-equal where `want` is a number, NaN where it is NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    iview = np.int32 if got.dtype == F else np.int64
    return bool(np.isnan(got[nan]).all() and (got.view(iview)[~nan] == want.view(iview)[~nan]).all())


class Rows:
    """the part of a decoder that PrototypeTracker.apply reads: class lists, a sample count, and a workspace that begins with one
    OlState per stream, of which only the unit rows are filled in"""
    device = torch.device("cuda:0")
    phase = 0

    def __init__(self, ids, rows, vote, multi=False):
        ids, rows = (ids, rows) if multi else ([ids], [rows])
        host = np.zeros((len(ids), OL_STATE), dtype=np.uint8)
        for s, r in enumerate(rows):
            if r is not None:
                b = np.ascontiguousarray(r, dtype=F).view(np.uint8).reshape(-1)
                host[s, OL_TABLE:OL_TABLE + b.size] = b
        self.ws = torch.from_numpy(host.reshape(-1)).cuda()
        cid = [None if i is None else torch.as_tensor(np.asarray(i), dtype=torch.int32) for i in ids]
        self.class_ids = cid if multi else cid[0]
        self.vote = vote
        self.n_seen = np.zeros(len(ids), dtype=np.int64) if multi else 0

    def push(self, *a, **k):
        raise AssertionError("apply() does not push the decoder")


def drifting(n, k, seed, with_bad_rows=True):
    emb, exp, rows = T.drifting_stream(n, k, seed=seed, noise=0.4, degrees=40.0, segment=20, rest_every=5)
    if with_bad_rows:
        emb = emb.copy()
        emb[7, 3], emb[40, 0], emb[41] = np.nan, np.inf, 0.0
        emb[150], emb[300, 15], emb[301, 2] = np.nan, -np.inf, np.nan
    return emb, exp, rows, np.arange(k) * 2 + 1


BAD_ROWS = [7, 40, 41, 150, 300, 301]
SETTINGS = dict(rate=0.1, min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.9)


def apply_cuts(tracker, emb, cuts):
    dev = torch.from_numpy(emb).cuda()
    outs, p = [], 0
    for n in cuts:
        outs.append(tracker.apply(dev[p:p + n], return_logits=True))
        p += n
    assert p == emb.shape[0]
    return [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(4)]


def assert_matches(got, state, want, what):
    pred, voted, logits, updated = got
    for name, g in (("pred", pred), ("voted", voted), ("updated", updated)):
        bad = np.nonzero(g.astype(np.int64) != want[name])[0]
        assert bad.size == 0, (what, name, bad[:5], g[bad[:5]], want[name][bad[:5]])
    assert same_floats(logits, want["logits"]), (what, "logits")
    ws = want["state"]
    assert np.array_equal(state["ids"], ws["ids"]) and state["ring"] == ws["ring"], (what, "ids / ring")
    assert np.array_equal(state["n_updates"], ws["n_updates"]) and np.array_equal(state["n_refused"], ws["n_refused"]), (what, "counters")
    for name in ("anchor", "rows", "acc"):
        assert same_bits(state[name], ws[name]), (what, name)


# ---------------------------------------------------------------------------------------------------------------------------
# the stage against the definition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agree", [False, True])
@pytest.mark.parametrize("vote", [1, 25, 256])
@pytest.mark.parametrize("K", [1, 2, 41, 64])
def test_stage_equals_the_definition_on_the_drifting_stream(K, vote, agree):
    emb, exp, rows, ids = drifting(640, K, seed=K)
    want = track_reference(emb, rows, ids, agree=agree, vote=vote, **SETTINGS)
    # the input makes the stage work: counted on the definition, before anything is compared
    n_up, n_ref = int(want["state"]["n_updates"].sum()), int(want["state"]["n_refused"].sum())
    print(K, vote, agree, n_up, n_ref)
    assert n_up >= 20 and (K > 2 or n_ref >= 20) and (want["updated"][BAD_ROWS] == -1).all()
    assert not same_bits(want["state"]["rows"], rows)
    tracker = PrototypeTracker(Rows(ids, rows, vote), agree=agree, vote=vote, **SETTINGS)
    got = apply_cuts(tracker, emb, (1, 16, 17, 255, emb.shape[0] - 289))
    assert_matches(got, tracker.state(), want, (K, vote, agree))
    r, i, nu, nr = tracker.rows()
    assert same_bits(r.cpu().numpy(), want["state"]["rows"]) and np.array_equal(i, ids)
    assert np.array_equal(nu, want["state"]["n_updates"]) and np.array_equal(nr, want["state"]["n_refused"])


def test_an_anchor_bound_under_one_refuses_everything_and_reset_goes_back_to_the_anchor():
    emb, exp, rows, ids = drifting(320, 5, seed=9)
    kw = dict(SETTINGS, agree=False, vote=9)
    held = PrototypeTracker(Rows(ids, rows, 9), **dict(kw, min_anchor_cosine=float(np.nextafter(F(1), F(0)))))
    got = apply_cuts(held, emb, (320,))
    st = held.state()
    assert (got[3] == -1).all() and st["n_updates"].sum() == 0 and st["n_refused"].sum() > 50 and same_bits(st["rows"], rows)
    free = PrototypeTracker(Rows(ids, rows, 9), **kw)
    apply_cuts(free, emb, (320,))
    assert not same_bits(free.state()["rows"], rows) and len(free.state()["ring"]) == 9
    free._dev_reset(-1, rows=False)                                    # the ring alone
    st = free.state()
    assert st["ring"] == [] and not same_bits(st["rows"], rows) and st["n_updates"].sum() > 0
    free._dev_reset(0, rows=True)
    st = free.state()
    assert same_bits(st["rows"], rows) and same_bits(st["acc"], rows.astype(np.float64)) and st["n_updates"].sum() == 0
    assert_matches(apply_cuts(free, emb, (320,)), free.state(), track_reference(emb, rows, ids, **kw), "after reset")


# ---------------------------------------------------------------------------------------------------------------------------
# cuts and neighbours
# ---------------------------------------------------------------------------------------------------------------------------
def test_any_cut_gives_the_same_outputs_and_state():
    emb, exp, rows, ids = drifting(700, 17, seed=4)
    kw = dict(SETTINGS, agree=True, vote=25)
    whole = PrototypeTracker(Rows(ids, rows, 25), **kw)
    want = apply_cuts(whole, emb, (700,))                              # (256 + 256 + 188 launches)
    rng = np.random.default_rng(8)
    for trial in range(3):
        cuts = []
        while sum(cuts) < 700:
            cuts.append(int(min(rng.choice([0, 1, 2, 15, 16, 17, 63, 64, 65, 300]), 700 - sum(cuts))))
        cut = PrototypeTracker(Rows(ids, rows, 25), **kw)
        got = apply_cuts(cut, emb, cuts)
        for g, w, name in zip(got, want, ("pred", "voted", "logits", "updated")):
            assert same_floats(g, w) if g.dtype == F else np.array_equal(g, w), (trial, name)
        a, b = cut.state(), whole.state()
        assert all(same_bits(a[k], b[k]) for k in ("rows", "acc", "n_updates", "n_refused")) and a["ring"] == b["ring"], trial


def test_256_streams_in_one_launch_each_equal_the_stream_alone():
    rng = np.random.default_rng(5)
    S, launches = 256, 10
    ks = rng.choice([1, 2, 3, 5, 17, 41, 64], S)
    ids = [np.sort(rng.choice(300, k, replace=False)) for k in ks]
    data = [T.drifting_stream(launches * 12, int(k), seed=100 + s, noise=0.4, degrees=40.0, segment=10) for s, k in enumerate(ks)]
    ids[9], ks[9] = None, 0                                            # one stream never has classes or rows
    m = rng.integers(0, 13, (launches, S)) * (rng.random((launches, S)) > 0.25)        # some streams sit a launch out
    m[:, 7] = 0                                                                       # and one never has a row
    m[:, 9] = 0
    kw = dict(SETTINGS, agree=True, vote=7)
    many = PrototypeTracker(Rows(ids, [None if i is None else d[2] for i, d in zip(ids, data)], 7, multi=True), **kw)
    pos = np.zeros(S, dtype=np.int64)
    outs = [[] for _ in range(S)]
    dev = [torch.from_numpy(d[0]).cuda() for d in data]
    for t in range(launches):
        res = many.apply([dev[s][pos[s]:pos[s] + m[t, s]] if m[t, s] else None for s in range(S)], return_logits=True)
        for s in range(S):
            outs[s].append(res[s])
        pos += m[t]
    assert many.ws.numel() >= S * T._OT_WORDS * 4
    for s in (0, 1, 2, 7, 100, 254, 255):
        n = int(pos[s])
        got = [torch.cat([o[i] for o in outs[s]]).cpu().numpy() for i in range(4)]
        alone = PrototypeTracker(Rows(ids[s], data[s][2], 7), **kw)
        want = apply_cuts(alone, data[s][0][:n], (n,)) if n else [g[:0] for g in got]
        for g, w, name in zip(got, want, ("pred", "voted", "logits", "updated")):
            assert g.shape == w.shape and (same_floats(g, w) if g.dtype == F else np.array_equal(g, w)), (s, name)
        a, b = many.state(s), alone.state()
        assert all(same_bits(a[k], b[k]) for k in ("ids", "anchor", "rows", "acc", "n_updates", "n_refused")) and a["ring"] == b["ring"], s
        assert_matches(got, a, track_reference(data[s][0][:n], data[s][2], ids[s], **kw), s)
    assert all(o[0].shape == (0,) for o in outs[9])


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


def _recordings(n, seed=11, length=6200):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((rng.standard_normal((length, 12)) * (1 + 0.2 * i) * 2e-3).astype(np.float32)).cuda()
            for i in range(n)]


@pytest.fixture(scope="module")
def norm():
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rec = _recordings(1, seed=5, length=3000)[0]
    w = preprocess_segments(rec[None], keep=20 * np.arange(140))[0]
    return w.mean(0), w.std(0)


# windows per push 1, 15, 16, 17, 256: window k is final once 20 k + 11 samples have arrived
CHUNKS = (21, 300, 320, 340, 5120)
WINDOWS = (1, 15, 16, 17, 256)
CLASSES = [list(range(41)), [30, 2, 17, 5, 9], [7]]
KINDS = ["single", "adapt", "multi", "multi_adapt"]


def make_decoder(kind, engine, norm, dtype, vote=9):
    from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, MultiStreamDecoder, OnlineDecoder
    mean, std = norm
    if kind in ("single", "adapt"):
        return OnlineDecoder(engine, mean, std, classes=CLASSES[1], vote=vote, dtype=dtype, adapt=0.01 if kind == "adapt" else None)
    S = len(CLASSES) + 1                                               # the last stream never gets classes or samples
    if kind == "multi":
        dec = MultiStreamDecoder(engine, mean, std, S, vote=vote, dtype=dtype)
    else:
        dec = AdaptiveMultiStreamDecoder(engine, mean, std, S, [0.0, 0.01, 0.02, 0.0], vote=vote, dtype=dtype)
    for s, c in enumerate(CLASSES):
        dec.set_classes(s, classes=c)
    return dec


def chunks_of(kind, recs, p, n):
    """push `n` samples from position p: of the single decoders' one stream, or of streams 0 and 1 (stream 2 sits every other push out)"""
    if kind in ("single", "adapt"):
        return recs[0][p:p + n]
    return [recs[0][p:p + n], recs[1][p:p + n], None, None]


def unit_rows(table):
    """a class table as `set_classes` normalises it: f32, the sum of squares in order, one square root, one division"""
    t = table.cpu().numpy().astype(F)
    ss = np.zeros(t.shape[0], dtype=F)
    for d in range(16):
        ss = ss + t[:, d] * t[:, d]
    return t / np.sqrt(ss)[:, None]


def host_logits(emb, rows):
    l = np.zeros((emb.shape[0], rows.shape[0]), dtype=F)
    for d in range(16):
        l = l + emb[:, d:d + 1] * rows[None, :, d]
    return l


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_push_gives_out_its_embeddings_and_changes_nothing_else(engine, norm, kind, dtype):
    recs = _recordings(2, seed=21)
    with_emb, plain = make_decoder(kind, engine, norm, dtype), make_decoder(kind, engine, norm, dtype)
    multi = kind.startswith("multi")
    p = 0
    for n, m in zip(CHUNKS, WINDOWS):
        a = with_emb.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True, return_embeddings=True)
        b = plain.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True)
        p += n
        for s, (ra, rb) in enumerate(zip(a, b) if multi else [(a, b)]):
            assert len(ra) == 5 and len(rb) == 4
            rows = m if not multi or s < 2 else 0
            assert ra[0].shape == (rows,) and ra[4].shape == (rows, 16) and ra[4].dtype == torch.float32
            for x, y, name in zip(ra, rb, ("pred", "voted", "logits", "windows")):
                assert x.dtype == y.dtype and same_bits(x.cpu().numpy(), y.cpu().numpy()), (kind, dtype, n, s, name)
            if rows:
                table, ids = with_emb.class_table(s) if multi else with_emb.class_table()
                emb = ra[4].cpu().numpy()
                assert same_bits(host_logits(emb, unit_rows(table)), ra[2].cpu().numpy()), (kind, dtype, n, s)
                assert np.abs(np.linalg.norm(emb.astype(np.float64), axis=1) - 1).max() < 1e-6
    # without the other optional outputs the embeddings come last all the same
    a = with_emb.push(chunks_of(kind, recs, p, 60), return_embeddings=True)
    b = plain.push(chunks_of(kind, recs, p, 60))
    for ra, rb in (zip(a, b) if multi else [(a, b)]):
        assert len(ra) == 3 and len(rb) == 2 and ra[2].shape == (ra[0].shape[0], 16) and torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_rate_zero_behind_a_decoder_is_the_decoder(engine, norm, kind, dtype):
    recs = _recordings(2, seed=31)
    tracked, plain = make_decoder(kind, engine, norm, dtype), make_decoder(kind, engine, norm, dtype)
    tracker = PrototypeTracker(tracked, rate=0.0)
    multi = kind.startswith("multi")
    rng = np.random.default_rng(2)
    p = 0
    while p < 3000:
        n = int(rng.integers(1, 900))
        a = tracker.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True)
        b = plain.push(chunks_of(kind, recs, p, n), return_logits=True, return_windows=True)
        p += n
        for s, (ra, rb) in enumerate(zip(a, b) if multi else [(a, b)]):
            assert len(ra) == 5
            for x, y, name in zip(ra, rb, ("pred", "voted", "logits", "windows")):
                assert x.shape == y.shape and x.dtype == y.dtype and same_bits(x.cpu().numpy(), y.cpu().numpy()), (kind, dtype, p, s, name)
            assert (ra[4] == -1).all() and ra[4].shape == ra[0].shape
    if multi:
        raw = torch.cat([recs[0][:400], recs[1][:100]])
        for d in (tracker, plain):
            d.reset()
        a, b = tracker.push_packed(raw, [400, 100, 0, 0], return_logits=True), plain.push_packed(raw, [400, 100, 0, 0], return_logits=True)
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) for x, y in zip(a, b))
        with pytest.raises(IndexError):
            tracker.rows(4)
    else:
        with pytest.raises(TypeError):
            tracker.push_packed(recs[0][:40], [40])
    # a push of the decoder behind the tracker's back is refused before anything is enqueued
    tracked.push(chunks_of(kind, recs, 0, 40))
    from contrastiveprosthetics_amd._lib import CpNativeError
    with pytest.raises(CpNativeError):
        tracker.push(chunks_of(kind, recs, 40, 40))
    tracker.reset()
    tracker.push(chunks_of(kind, recs, 0, 40))


@pytest.mark.parametrize("kind", ["single", "multi_adapt"])
def test_tracking_behind_a_decoder_equals_the_definition_and_adopt_keeps_the_rows(engine, norm, kind):
    recs = _recordings(2, seed=41)
    dec = make_decoder(kind, engine, norm, "f32")
    multi = kind.startswith("multi")
    s = 1 if multi else 0
    kw = dict(rate=0.1, min_cosine=-2.0, min_margin=0.0, min_anchor_cosine=-2.0, agree=False)
    tracker = PrototypeTracker(dec, **kw)
    embs, outs = [], []
    for p in range(0, 2000, 500):
        if multi:
            res = dec.push(chunks_of(kind, recs, p, 500), return_embeddings=True)
            embs.append(res[s][-1])
            outs.append(tracker.apply([r[-1] for r in res], return_logits=True)[s])
        else:
            res = dec.push(chunks_of(kind, recs, p, 500), return_embeddings=True)
            embs.append(res[-1])
            outs.append(tracker.apply(res[-1], return_logits=True))
    emb = torch.cat(embs).cpu().numpy()
    assert emb.shape[0] == 100
    got = [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(4)]
    anchor = tracker.state(s)["anchor"]
    table, ids = dec.class_table(s) if multi else dec.class_table()
    assert same_bits(anchor, unit_rows(table))                        # the decoder's unit rows, bit for bit
    want = track_reference(emb, anchor, ids.numpy(), vote=dec.vote, **kw)
    assert want["state"]["n_updates"].sum() == 100
    assert_matches(got, tracker.state(s), want, kind)
    # adopt: the decoder takes the tracked rows (it normalises them once more: the last bit may move), the tracker the
    # decoder's as its new anchor, and from there the two agree bit for bit
    tracked = tracker.state(s)["rows"]
    tracker.adopt(s)
    table, ids2 = dec.class_table(s) if multi else dec.class_table()
    assert same_bits(table.cpu().numpy(), tracked) and np.array_equal(ids2.numpy(), ids.numpy())
    st = tracker.state(s)
    assert same_bits(st["anchor"], unit_rows(table)) and same_bits(st["rows"], st["anchor"]) and st["n_updates"].sum() == 0
    # (|tracked row|^2 is 1 within 2^-23; its f32 sum of squares adds at most 32 roundings of 2^-24 each, so the norm is 1
    # within 2^-20 and a component moves by at most that, plus one rounding)
    assert np.abs(st["anchor"] - tracked).max() <= 2.0 ** -19 and not same_bits(tracked, anchor)
    res = dec.push(chunks_of(kind, recs, 2000, 500), return_logits=True, return_embeddings=True)
    if multi:
        nxt, res = tracker.apply([r[-1] for r in res], return_logits=True)[s], res[s]
    else:
        nxt = tracker.apply(res[-1], return_logits=True)
    assert res[2].shape[0] == 25
    # the plain push's logits of the next window are the tracker's; behind it the tracker's rows have moved again
    assert same_bits(nxt[2][0].cpu().numpy(), res[2][0].cpu().numpy()) and nxt[0][0] == res[0][0]
    assert not same_bits(nxt[2][1:].cpu().numpy(), res[2][1:].cpu().numpy())


def test_the_gate_follows_the_trackers_logits():
    from contrastiveprosthetics_amd.online import CommandGate
    emb, exp, rows, ids = drifting(600, 12, seed=6, with_bad_rows=False)
    dec = Rows(ids, rows, 25)
    tracker = PrototypeTracker(dec, agree=True, vote=25, **SETTINGS)
    gate = CommandGate(dec, vote=25)
    dev = torch.from_numpy(emb).cuda()
    p, n_upd = 0, 0
    for n in (1, 40, 256, 303):
        pred, voted, logits, updated = tracker.apply(dev[p:p + n], return_logits=True)
        command, accepted, conf, margin = gate.apply(logits)
        assert torch.equal(command, voted) and torch.equal(accepted, pred), p
        n_upd += int((updated >= 0).sum())
        p += n
    assert n_upd > 50


# ---------------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------------
GRID = [dict(rate=0.0, vote=25), dict(rate=0.1, agree=False, vote=1, min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.9),
        dict(rate=0.05, agree=True, vote=25, min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.5),
        dict(rate=0.3, agree=True, vote=256, min_cosine=0.2, min_margin=0.0, min_anchor_cosine=0.8),
        dict(rate=0.02, agree=False, vote=7, min_cosine=0.5, min_margin=0.1, min_anchor_cosine=float(np.nextafter(F(1), F(0)))),
        dict()]


@pytest.fixture(scope="module")
def recording():
    emb, exp, rows, ids = drifting(3000, 8, seed=12)
    exp = np.where(exp >= 0, ids[np.maximum(exp, 0)], exp)
    exp[100:130] = T.IGNORE
    return emb, exp, rows, ids, {}


@pytest.mark.parametrize("n_configs,n_rows", [(1, 3000), (63, 255), (64, 256), (65, 257), (1000, 1), (1000, 257), (6, 3000)])
def test_sweep_equals_the_definition_and_the_stage(recording, n_configs, n_rows):
    emb, exp, rows, ids, cache = recording
    emb, exp = emb[:n_rows], exp[:n_rows]
    configs = [GRID[(g + (n_configs == 1)) % len(GRID)] for g in range(n_configs)]
    scores, pred, voted, updated = sweep_tracker(torch.from_numpy(emb).cuda(), exp, ids, rows, configs, return_sequences=True)
    assert pred.shape == (n_configs, n_rows) and pred.dtype == torch.int32
    pred, voted, updated = pred.cpu().numpy(), voted.cpu().numpy(), updated.cpu().numpy()
    for g, c in enumerate(configs):
        key = (n_rows, g % len(GRID) if n_configs > 1 else 1)
        if key not in cache:
            cache[key] = track_reference(emb, rows, ids, expected=exp, **c)
        want = cache[key]
        assert {k: int(scores[k][g]) for k in T.TRACK_SCORE_KEYS} == want["scores"], (g, c)
        assert np.array_equal(pred[g], want["pred"]) and np.array_equal(voted[g], want["voted"]) and np.array_equal(updated[g], want["updated"]), g
    only = sweep_tracker(torch.from_numpy(emb).cuda(), exp, ids, rows, configs)
    assert all(np.array_equal(only[k], scores[k]) for k in T.TRACK_SCORE_KEYS)
    for g in sorted({0, n_configs // 2, n_configs - 1}):              # the shipped stage, fresh, with that setting
        s = T._settings(configs[g])
        tracker = PrototypeTracker(Rows(ids, rows, s["vote"]), **s)
        got = apply_cuts(tracker, emb, (n_rows,))
        assert np.array_equal(got[0], pred[g]) and np.array_equal(got[1], voted[g]) and np.array_equal(got[3], updated[g]), g


def test_sweep_picks_a_tracking_setting_on_the_drifting_stream():
    emb, exp, rows = T.drifting_stream(**DRIFT)
    ids = np.arange(DRIFT["k"])
    configs = T.track_grid(rate=[0.0, 0.02, 0.05, 0.1], agree=[True, False])
    configs = [dict(DRIFT_SETTINGS, **c) for c in configs]
    scores = sweep_tracker(torch.from_numpy(emb).cuda(), exp, ids, rows, configs)
    g = T.pick_tracker(scores)
    print({k: scores[k].tolist() for k in T.TRACK_SCORE_KEYS}, g)
    assert g is not None and configs[g]["rate"] > 0.0
    assert scores["voted_hit_tail"][g] > scores["voted_hit_tail"][0] and scores["wrong_updates"][g] <= 0.02 * scores["updates"][g]
    want = track_reference(emb, rows, ids, expected=exp, **configs[g])["scores"]
    assert {k: int(scores[k][g]) for k in T.TRACK_SCORE_KEYS} == want


def test_embed_recording_is_a_fresh_streams_embeddings(engine, norm):
    rec = _recordings(1, seed=51, length=1500)[0]
    dec = make_decoder("single", engine, norm, "f32")
    dec.push(rec[:333])                                                # a stream in progress is reset, before and after
    emb = T.embed_recording(dec, rec)
    assert emb.shape == (75, 16) and dec.n_seen == 0
    again = dec.push(rec, return_embeddings=True)[-1]
    assert torch.equal(emb, again)
    multi = make_decoder("multi", engine, norm, "f32")
    assert torch.equal(T.embed_recording(multi, rec, 1), emb) and multi.n_seen[1] == 0
