"""The electrode map on the MI355X (contrastiveprosthetics_amd/online.py set_channel_map / score_channel_maps, csrc/online.cuh
ol_frontend_run, csrc/online_maps.cuh).  The contract is exact, so every comparison is torch.equal / ==: a mapped decoder on raw
against an unmapped one on raw[:, src] for all four decoders and any cut into pushes, masked channels, the wrappers and
recordings behind a map, the device sweep against its definition (fresh mapped decoders pushing the recording), the recovery of
a rotated sleeve, and the launch count of a mapped push."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
IDS = [2, 5, 9, 14, 20, 27, 33, 40]          # the 8 grasps of this user
PERM = np.array([3, 0, 7, 1, 11, 4, 2, 9, 5, 10, 8, 6], dtype=np.int32)         # a permutation that moves every channel
PERM2 = np.array([1, 2, 3, 4, 5, 6, 7, 0, 9, 8, 11, 10], dtype=np.int32)
COPY = np.array([0, 1, 2, 3, 4, 4, 6, 7, 8, 9, 10, 11], dtype=np.int32)         # no permutation: channel 5 copied from 4
ALPHA = 0.02
KINDS = ("single", "adapt", "multi", "multi_adapt")


def _train_steps(e, steps, seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(41).repeat(4).cuda()
    for _ in range(steps):
        x = (torch.randn(4 * 41, 12, generator=g) * 1.5 + 0.3).cuda()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(PARAMS)


def _engine(adabn=False, seed=3, steps=3):
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=adabn, dtype="f32", device="cuda:0", seed=seed)
    e.init_parameters(seed)
    _train_steps(e, steps, seed)
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def engine():
    return _engine()


@pytest.fixture(scope="module")
def ada():
    return _engine(True, seed=5)


def _amplitudes():
    """Per class a pattern of channel amplitudes.  Class i of the 8 is loud on ring electrode i and half as loud three places
    on, quiet on the rest of the ring: turned by s places, the pattern of class i is that of class i + s, so a wrong rotation
    decodes as another grasp rather than as noise.  The four electrodes off the ring tell pairs of classes apart."""
    amp = {-1: np.ones(12)}
    for i, c in enumerate(IDS):
        a = np.full(12, 0.3)
        a[i] = 6.0
        a[(i + 3) % 8] = 3.0
        a[8:] = [1.0 + 0.5 * (i % 2), 1.0 + 0.5 * (i // 4), 1.0, 1.0]
        amp[c] = a
    return amp


def _cued(seed):
    """A cued recording of the 8 classes: cue blocks of 560..640 samples in a shuffled order, unlabelled gaps between them;
    noise whose channel amplitudes follow the cue.  raw (n, 12) f32 on the GPU, labels (n,) int64."""
    rng = np.random.default_rng(seed)
    amp = _amplitudes()
    labels = [np.full(int(rng.integers(30, 120)), -1)]
    for c in rng.permutation(IDS):
        labels += [np.full(int(rng.integers(560, 640)), int(c)), np.full(int(rng.integers(30, 120)), -1)]
    labels = np.concatenate(labels).astype(np.int64)
    scale = np.stack([amp[int(c)] for c in labels])
    raw = (rng.standard_normal((labels.shape[0], 12)) * scale * 2e-3).astype(np.float32)
    return torch.from_numpy(raw).cuda(), labels


@pytest.fixture(scope="module")
def cued():
    from contrastiveprosthetics_amd.online import windows_before
    raw, labels = _cued(31)
    m = windows_before(raw.shape[0])
    assert 250 <= m <= 320 and m % 16 != 0, m                          # ragged against the 16-row tiles
    return raw, labels


@pytest.fixture(scope="module")
def second():
    """another recording of the same patterns: what the user enrols and calibrates from"""
    return _cued(32)


@pytest.fixture(scope="module")
def norm(cued):
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    w = preprocess_segments(cued[0][None], keep=20 * np.arange(256))[0]
    return w.mean(0), w.std(0)


def _cuts(n, how):
    if how == "random":
        rng = np.random.default_rng(7)
        out = []
        while sum(out) < n:
            out.append(int(rng.integers(1, 700)))
        out[-1] -= sum(out) - n
        return out
    return [how] * (n // how) + ([n % how] if n % how else [])


def _make(kind, engine, ada, norm, second, dtype, maps=(None, None, None), **kw):
    """a decoder of the kind with the 8 classes, calibrated (adaptive forms) before any map is set; multi forms: 3 streams"""
    from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, MultiStreamDecoder, OnlineDecoder
    mean, std = norm
    if kind == "single":
        d = OnlineDecoder(engine, mean, std, classes=IDS, dtype=dtype, **kw)
    elif kind == "adapt":
        alpha = kw.pop("adapt", ALPHA)
        d = OnlineDecoder(ada, mean, std, classes=IDS, dtype=dtype, adapt=alpha, **kw)
        d.calibrate(second[0])
    else:
        d = MultiStreamDecoder(engine, mean, std, 3, dtype=dtype, **kw) if kind == "multi" \
            else AdaptiveMultiStreamDecoder(ada, mean, std, 3, ALPHA, dtype=dtype, **kw)
        for s in range(3):
            d.set_classes(s, IDS)
            if kind == "multi_adapt":
                d.calibrate(s, second[0])
    if kind in ("single", "adapt"):
        if maps[0] is not None:
            d.set_channel_map(*maps[0])
    else:
        for s in range(3):
            if maps[s] is not None:
                d.set_channel_map(s, *maps[s])
    return d


def _run(dec, raws, cuts):
    """push the recording(s) cut into pushes; per stream (pred, voted, logits, windows) concatenated"""
    multi = hasattr(dec, "n_streams")
    outs = []
    s = 0
    for n in cuts:
        if multi:
            outs.append(dec.push([r[s:s + n] for r in raws], return_logits=True, return_windows=True))
        else:
            outs.append([dec.push(raws[0][s:s + n], return_logits=True, return_windows=True)])
        s += n
    assert s == raws[0].shape[0]
    return [tuple(torch.cat([o[st][i] for o in outs]) for i in range(4)) for st in range(len(outs[0]))]


def _same(got, want, what):
    for name, g, w in zip(("pred", "voted", "logits", "windows"), got, want):
        assert g.shape == w.shape and torch.equal(g, w), (what, name)


def _cols(raw, src):
    return raw[:, torch.as_tensor(np.asarray(src), dtype=torch.long, device=raw.device)].contiguous()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.fixture(scope="module")
def unmapped(engine, ada, norm, second, cued):
    """per (kind, dtype): what an unmapped decoder makes of raw[:, src] per stream, pushed whole.  A stream's outputs do not
    depend on the cut (tests/test_gpu_online*.py), so one reference serves every cut."""
    cache = {}

    def get(kind, dtype):
        if (kind, dtype) not in cache:
            raw = cued[0]
            raws = [_cols(raw, PERM)] if kind in ("single", "adapt") else [raw, _cols(raw, PERM), _cols(raw, PERM2)]
            cache[kind, dtype] = _run(_make(kind, engine, ada, norm, second, dtype), raws, [raw.shape[0]])
        return cache[kind, dtype]
    return get


@pytest.mark.parametrize("cut", [1, 19, 333, "random"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_mapped_push_equals_an_unmapped_push_of_permuted_raw(engine, ada, norm, second, cued, unmapped, kind, dtype, cut):
    """multi forms: stream 0 unmapped, streams 1 and 2 under two different maps, all three fed the same raw"""
    raw = cued[0]
    single = kind in ("single", "adapt")
    maps = [(PERM,), None, None] if single else [None, (PERM,), (PERM2,)]
    dec = _make(kind, engine, ada, norm, second, dtype, maps)
    got = _run(dec, [raw] if single else [raw] * 3, _cuts(raw.shape[0], cut))
    want = unmapped(kind, dtype)
    assert len(got) == len(want) and got[0][0].shape[0] == want[0][0].shape[0] > 250
    for s, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (kind, dtype, cut, s))
    if not single:                                                      # and the maps did something
        assert not torch.equal(got[0][3], got[1][3]) and not torch.equal(got[1][3], got[2][3])


@pytest.mark.parametrize("kind", ["single", "adapt"])
def test_identity_no_map_and_a_copied_channel(engine, ada, norm, second, cued, kind):
    raw = cued[0]
    cuts = _cuts(raw.shape[0], 333)
    never = _run(_make(kind, engine, ada, norm, second, "f32"), [raw], cuts)[0]
    ident = _make(kind, engine, ada, norm, second, "f32", [(np.arange(12),), None, None])
    assert ident.channel_map()[0].tolist() == list(range(12))
    _same(_run(ident, [raw], cuts)[0], never, "identity")
    cleared = _make(kind, engine, ada, norm, second, "f32", [(PERM,), None, None])
    cleared.set_channel_map(None)
    assert cleared.channel_map() is None
    _same(_run(cleared, [raw], cuts)[0], never, "src=None")
    copied = _make(kind, engine, ada, norm, second, "f32", [(COPY,), None, None])
    got = _run(copied, [raw], cuts)[0]
    _same(got, _run(_make(kind, engine, ada, norm, second, "f32"), [_cols(raw, COPY)], cuts)[0], "channel 5 from 4")
    assert not torch.equal(got[3], never[3])


def test_multi_stream_maps_are_per_stream_and_survive_reset_refresh_and_set_classes(engine, ada, norm, second, cued):
    raw = cued[0][:2000]
    dec = _make("multi", engine, ada, norm, second, "f32", [None, (PERM,), (PERM2, 0.5)])
    assert dec.channel_map(0) is None and dec.channel_map(1)[0].tolist() == PERM.tolist() and dec.channel_map(2)[1].tolist() == [0.5] * 12
    first = _run(dec, [raw] * 3, [2000])
    dec.reset()
    dec.refresh()
    for s in range(3):
        dec.set_classes(s, IDS)
    again = _run(dec, [raw] * 3, [700, 1300])
    for s in range(3):
        _same(again[s], first[s], s)
    dec.set_channel_map(1, None)                                        # back to the identity: as stream 0
    dec.reset()
    out = _run(dec, [raw] * 3, [2000])
    _same(out[1], out[0], "cleared")
    _same(out[2], first[2], "the others keep theirs")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_masked_channels_emit_their_fill_and_the_rest_is_untouched(engine, ada, norm, second, cued, dtype):
    """The reference for pred is an unmapped decoder whose windows are identical by construction: std = inf on channel 2 makes
    (r - 0) / inf == +0, and mean = -0.25 * 2^100, std = 2^100 on channel 9 make (r + 2^98) / 2^100 == 0.25 exactly (r is
    far below half an ulp of 2^98)."""
    from contrastiveprosthetics_amd.online import OnlineDecoder
    raw = cued[0]
    mean, std = norm
    src = np.arange(12)
    src[[2, 9]] = -1
    fill = np.zeros(12, dtype=np.float32)
    fill[9] = 0.25
    fill[4] = 3.0                                                       # not masked: never read
    cuts = _cuts(raw.shape[0], 333)
    plain = _run(_make("single", engine, ada, norm, second, dtype), [raw], cuts)[0]
    dec = _make("single", engine, ada, norm, second, dtype, [(src, fill), None, None])
    got = _run(dec, [raw], cuts)[0]
    w = got[3]
    assert w.shape[0] > 250
    assert torch.equal(w[:, 2], torch.zeros_like(w[:, 2])) and torch.equal(w[:, 9], torch.full_like(w[:, 9], 0.25))
    keep = torch.as_tensor([c for c in range(12) if c not in (2, 9)]).cuda()
    assert torch.equal(w[:, keep], plain[3][:, keep])
    m2, s2 = mean.clone(), std.clone()
    m2[2], s2[2] = 0.0, float("inf")
    m2[9], s2[9] = -0.25 * 2.0 ** 100, 2.0 ** 100
    twin = OnlineDecoder(engine, m2, s2, classes=IDS, dtype=dtype)
    want = _run(twin, [raw], cuts)[0]
    _same(got, want, "the unmapped decoder with the same windows")
    assert not torch.equal(got[2], plain[2])                            # the mask changes the logits
    # unmask, reset: a fresh decoder (the masked channels' filters ran on zeros; reset clears them)
    dec.set_channel_map(None)
    dec.reset()
    _same(_run(dec, [raw], cuts)[0], plain, "unmasked and reset")


def test_unmasking_in_mid_stream_settles_after_a_transient(engine, ada, norm, second, cued):
    """not part of the exact contract: documents that a map changed in mid-stream leaves a filter transient and no more"""
    raw = cued[0]
    src = np.arange(12)
    src[2] = -1
    dec = _make("single", engine, ada, norm, second, "f32", [(src,), None, None])
    plain = _run(_make("single", engine, ada, norm, second, "f32"), [raw], [raw.shape[0]])[0]
    a = dec.push(raw[:3000], return_windows=True)[2]
    dec.set_channel_map(None)
    b = dec.push(raw[3000:], return_windows=True)[2]
    w = torch.cat([a, b])
    keep = torch.as_tensor([c for c in range(12) if c != 2]).cuda()
    assert torch.equal(w[:, keep], plain[3][:, keep])                   # the other channels never noticed
    tail = slice(a.shape[0] + 50, None)                                 # 1000 samples on, an order-4 Butterworth has settled
    assert torch.allclose(w[tail, 2], plain[3][tail, 2], rtol=1e-3, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------- 3
def _profile():
    f = np.float32
    k = len(IDS)
    return dict(ids=np.array(IDS, dtype=np.int64), rest=np.full(12, -0.5, f), span=np.full((k, 12), 2.0, f),
                weight=np.tile(np.arange(1, 13, dtype=np.int32) * 20, (k, 1)), low=np.full(12, -0.9, f), high=np.full(12, 1.5, f))


@pytest.mark.parametrize("kind", ["single", "multi"])
def test_gate_and_drive_over_a_mapped_decoder(engine, ada, norm, second, cued, kind):
    from contrastiveprosthetics_amd.online import CommandGate, GraspDrive
    raw = cued[0]
    single = kind == "single"
    maps = [(PERM,), None, None] if single else [None, (PERM,), (PERM2,)]
    raws = [_cols(raw, PERM)] if single else [raw, _cols(raw, PERM), _cols(raw, PERM2)]
    prof = _profile() if single else [_profile()] * 3
    outs = []
    for mp, rr in ((maps, [raw] * len(raws)), ([None] * 3, raws)):
        dec = _make(kind, engine, ada, norm, second, "f32", mp)
        drive = GraspDrive(CommandGate(dec, dwell=3, min_margin=0.01), profile=prof, smooth=5, bad_after=3, good_after=10)
        res = []
        s = 0
        for n in _cuts(raw.shape[0], 777):
            r = drive.push(rr[0][s:s + n] if single else [x[s:s + n] for x in rr], return_logits=True, return_windows=True)
            res.append([r] if single else r)
            s += n
        outs.append([tuple(torch.cat([o[st][i] for o in res]) for i in range(len(res[0][st]))) for st in range(len(res[0]))])
    got, want = outs
    for st in range(len(got)):
        assert len(got[st]) == len(want[st]) == 11                      # pred voted logits windows command accepted conf margin drive active bad
        for i, (g, w) in enumerate(zip(got[st], want[st])):
            assert torch.equal(g, w), (st, i)


@pytest.mark.parametrize("kind", KINDS)
def test_enroll_and_calibrate_on_a_mapped_decoder(engine, ada, norm, second, cued, kind):
    """a permutation against an unmapped decoder on raw[:, src]; a permutation with one masked channel against a decoder that
    only masks, on the host-permuted raw (what the mask itself does is the test above)"""
    raw2, lab2 = second
    single = kind in ("single", "adapt")
    st = () if single else (1,)
    masked = PERM.copy()
    masked[6] = -1
    only_mask = np.arange(12)
    only_mask[6] = -1
    fill = np.full(12, 0.125, dtype=np.float32)

    def make(m):
        return _make(kind, engine, ada, norm, second, "f32", [m, None, None] if single else [None, m, None])

    plain = make(None)
    plain.enroll(*st, raw2, lab2)
    for src, mine, twins in ((PERM, (PERM, None), None), (masked, (masked, fill), (only_mask, fill))):
        host = _cols(raw2, np.where(src < 0, 0, src))                    # (the masked column: any finite signal)
        mapped, twin = make(mine), make(twins)
        if kind in ("adapt", "multi_adapt"):
            mapped.calibrate(*st, raw2)
            twin.calibrate(*st, host)
            assert torch.equal(mapped.bn_statistics(*st), twin.bn_statistics(*st))
            assert not torch.equal(mapped.bn_statistics(*st), plain.bn_statistics(*st))
        mapped.enroll(*st, raw2, lab2)
        twin.enroll(*st, host, lab2)
        (ta, ia), (tb, ib) = mapped.class_table(*st), twin.class_table(*st)
        assert torch.equal(ta, tb) and torch.equal(ia, ib)
        assert not torch.equal(ta, plain.class_table(*st)[0])


def test_recording_windows_under_a_map(engine, ada, norm, second, cued):
    from contrastiveprosthetics_amd.online import recording_windows
    raw = cued[0]
    dec = _make("single", engine, ada, norm, second, "f32", [(PERM,), None, None])
    w = recording_windows(raw, dec.mean_std, channel_map=(PERM, None))
    assert torch.equal(w, recording_windows(_cols(raw, PERM), dec.mean_std))
    assert torch.equal(w, dec.push(raw, return_windows=True)[2])
    ada_dec = _make("adapt", engine, ada, norm, second, "f32", [(PERM,), None, None])
    assert torch.equal(ada_dec.calibration_windows(raw), w)             # the offline path under the map


# ---------------------------------------------------------------------------------------------------------------- 4
def _sweep_maps():
    from contrastiveprosthetics_amd.online import leave_one_out, rotations
    maps = np.concatenate([rotations(), leave_one_out(), COPY[None]])
    fills = np.zeros(maps.shape, dtype=np.float32)
    fills[8:20] = 0.25 * (np.arange(12)[:, None] - 5)                   # a fill per leave-one-out map
    assert maps.shape == (21, 12)
    return maps, fills


def _by_definition(fresh, raw, labels, maps, fills):
    """score_channel_maps as its docstring defines it: fresh mapped decoders push the recording; counted in numpy"""
    from contrastiveprosthetics_amd.online import window_labels
    wl = window_labels(labels, 0)
    ids = np.array(IDS)
    scored = np.isin(wl, ids)
    preds, voteds, scores = [], [], []
    for g in range(maps.shape[0]):
        dec, stream = fresh()
        if stream is None:
            dec.set_channel_map(maps[g], fills[g])
            p, v = dec.push(raw)
        else:
            dec.set_channel_map(stream, maps[g], fills[g])
            chunks = [None] * dec.n_streams
            chunks[stream] = raw
            p, v = dec.push(chunks)[stream]
        p, v = p.cpu().numpy(), v.cpu().numpy()
        preds.append(p)
        voteds.append(v)
        scores.append(dict(rows=int(scored.sum()), raw_hits=int((p == wl)[scored].sum()), voted_hits=int((v == wl)[scored].sum()),
                           per_class_voted_hits=np.array([int(((v == wl) & (wl == c)).sum()) for c in ids])))
    return scores, np.stack(preds), np.stack(voteds)


def _assert_scores(got, want, what):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        for k in ("rows", "raw_hits", "voted_hits"):
            assert a[k] == b[k], (what, g, k, a[k], b[k])
        assert np.array_equal(a["per_class_voted_hits"], b["per_class_voted_hits"]), (what, g)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["single", "multi", "adapt"])
def test_sweep_equals_its_definition(engine, ada, norm, second, cued, kind, dtype):
    from contrastiveprosthetics_amd.online import score_channel_maps
    raw, labels = cued
    raw2, lab2 = second
    maps, fills = _sweep_maps()
    stream = 1 if kind == "multi" else None
    dec = _make(kind, engine, ada, norm, second, dtype)
    dec.enroll(raw2, lab2) if stream is None else dec.enroll(stream, raw2, lab2)            # the rows belong to this user
    table = dec.class_table() if stream is None else dec.class_table(stream)
    if kind == "adapt":
        stats = dec.bn_statistics()

    def fresh():
        if kind == "adapt":                                            # alpha = 0 on a copy of the statistics
            d = _make(kind, engine, ada, norm, second, dtype, adapt=0.0)
            assert torch.equal(d.bn_statistics(), stats)
        else:
            d = _make(kind, engine, ada, norm, second, dtype)
        d.set_classes(table=table[0], ids=table[1]) if stream is None else d.set_classes(stream, table=table[0], ids=table[1])
        return d, stream

    want, wp, wv = _by_definition(fresh, raw, labels, maps, fills)
    assert want[0]["rows"] > 150 and len({s["voted_hits"] for s in want}) > 3          # the maps differ in what they score
    results = {}
    for chunk in (48, 1000, None):                                      # chunk edges inside maps; the default: one chunk
        got, pred, voted = score_channel_maps(dec, raw, labels, maps, fills, stream=stream, return_pred=True, chunk_rows=chunk,
                                              per_class=True)
        assert pred.dtype == voted.dtype == torch.int32 and tuple(pred.shape) == tuple(voted.shape) == wp.shape
        assert np.array_equal(pred.cpu().numpy(), wp), (kind, dtype, chunk)
        assert np.array_equal(voted.cpu().numpy(), wv), (kind, dtype, chunk)
        _assert_scores(got, want, (kind, dtype, chunk))
        results[chunk] = (got, pred, voted)
    for chunk in (48, 1000):                                            # the results do not depend on chunk_rows
        assert torch.equal(results[chunk][1], results[None][1]) and torch.equal(results[chunk][2], results[None][2])
    # the sweep left the decoder's live stream alone
    if stream is None:
        assert dec.n_seen == 0
        if kind == "adapt":
            assert torch.equal(dec.bn_statistics(), stats)
    plain = score_channel_maps(dec, raw, labels, maps, fills, stream=stream)
    assert [(s["rows"], s["raw_hits"], s["voted_hits"]) for s in plain] == [(s["rows"], s["raw_hits"], s["voted_hits"]) for s in want]
    assert "per_class_voted_hits" not in plain[0]


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sweep_recovers_a_rotated_sleeve(engine, ada, norm, second, cued, dtype):
    from contrastiveprosthetics_amd.online import pick_channel_map, rotations, score_channel_maps
    raw, labels = cued
    raw2, lab2 = second
    rot = rotations()
    dec = _make("single", engine, ada, norm, second, dtype)
    dec.enroll(raw2, lab2)
    base = score_channel_maps(dec, raw, labels, rot[:1], per_class=True)[0]              # the sleeve as it was enrolled
    turned = _cols(raw, rot[3])                                         # the sleeve back on, three places round
    scores = score_channel_maps(dec, turned, labels, rot, per_class=True)
    inverse = 5
    assert rot[3][rot[inverse]].tolist() == list(range(12))
    for k in ("rows", "raw_hits", "voted_hits"):
        assert scores[inverse][k] == base[k], k
    assert np.array_equal(scores[inverse]["per_class_voted_hits"], base["per_class_voted_hits"])
    assert pick_channel_map(scores) == inverse
    for g in range(8):
        if g != inverse:
            assert scores[g]["voted_hits"] < scores[inverse]["voted_hits"], (g, scores[g], scores[inverse])
    assert 2 * base["voted_hits"] > base["rows"]                        # and the enrolled user is decoded at all
    dec.set_channel_map(rot[inverse])
    p, v = dec.push(turned)
    fresh = _make("single", engine, ada, norm, second, dtype)
    fresh.set_classes(table=dec.class_table()[0], ids=dec.class_table()[1])
    p0, v0 = fresh.push(raw)
    assert torch.equal(p, p0) and torch.equal(v, v0)


# ---------------------------------------------------------------------------------------------------------------- 6
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


@pytest.mark.parametrize("kind", KINDS)
def test_a_mapped_push_adds_no_launch(engine, ada, norm, second, cued, kind):
    raw = cued[0]
    single = kind in ("single", "adapt")
    plain = _make(kind, engine, ada, norm, second, "f32")
    mapped = _make(kind, engine, ada, norm, second, "f32", [(PERM,), None, None] if single else [None, (PERM,), (PERM2,)])
    chunk = raw[:500] if single else [raw[:500]] * 3
    for d in (plain, mapped):
        d.push(chunk)                                                   # (the counts' device copy is made once)
    a = _count_kernels(lambda: plain.push(chunk))
    b = _count_kernels(lambda: mapped.push(chunk))
    assert a == b and a >= 10, (a, b)
