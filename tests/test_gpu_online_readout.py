"""The closed-form head fit on the MI355X (contrastiveprosthetics_amd/readout.py, csrc/online_readout.cuh) against the numpy
definitions: the moments and the solve in every bit, the apply against the embeddings of a push with the projection installed,
the chain from a cued recording to `pick_ridge`'s integer tables, and a stream of a multi-stream decoder."""
import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import readout as R
from contrastiveprosthetics_amd._lib import CpNativeError
from contrastiveprosthetics_amd.online import MultiStreamDecoder, OnlineDecoder, window_labels, windows_before
from test_gpu_online_track import _engine
from test_online_readout_host import same_bits, small_case

pytestmark = pytest.mark.gpu

F = np.float32
IDS = [2, 5, 9, 17]
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def engine():
    return _engine()


def on_gpu(u, dtype):
    return torch.from_numpy(u).cuda().to(TORCH[dtype])


# ---------------------------------------------------------------------------------------------------------------------------
# moments and solve against the definition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("balanced", [True, False])
@pytest.mark.parametrize("n", [1, R.STAGE - 1, R.STAGE, R.STAGE + 1, 100])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_moments_equal_the_definition_in_every_bit(dtype, n, balanced):
    """three groups of which group 1 is empty, windows with a negative slot among the rest"""
    u, slots, groups, targets = small_case(n, k=3, seed=10 + n, n_groups=3, bf16=dtype == "bf16")
    groups[groups == 1] = 2
    if n >= R.STAGE - 1:
        assert (slots < 0).any() and (slots >= 0).any()
    w = R.window_weights(slots, 3, balanced, groups)
    want_g, want_c = R.moments_reference(u, slots, w, targets, groups, 3)
    G, Cm = R.moments(on_gpu(u, dtype), slots, w, targets, groups, 3)
    got_g, got_c = G.cpu().numpy(), Cm.cpu().numpy()
    assert not want_g[1].any() and not want_c[1].any()
    assert same_bits(got_g, want_g), ("G", np.abs(got_g - want_g).max())
    assert same_bits(got_c, want_c), ("C", np.abs(got_c - want_c).max())


def test_an_empty_recording_gives_zero_moments():
    G, Cm = R.moments(torch.empty(0, 512, device="cuda"), np.zeros(0, np.int64), np.zeros(0), np.eye(2, 16, dtype=F), None, 2)
    assert not G.cpu().numpy().any() and not Cm.cpu().numpy().any()


@pytest.fixture(scope="module")
def moments100():
    u, slots, groups, targets = small_case(100, k=3, seed=1, n_groups=3)
    groups[groups == 1] = 2                                    # group 1 is empty: a plan on it alone has nothing to fit
    w = R.window_weights(slots, 3, True, groups)
    G, Cm = R.moments_reference(u, slots, w, targets, groups, 3)
    return G, Cm


def test_four_plans_and_one_that_fails_in_one_call(moments100):
    """two masks x two ridges with 100 windows < 513 unknowns, so that only the ridge makes the matrix definite; a fifth plan
    on the empty group with ridge 0 fails at the first pivot and leaves the others alone"""
    G, Cm = moments100
    plans = [((0, 2), 1e-4), ((0, 2), 1.0), ((0,), 1e-4), ((0,), 1.0)]
    want = R.solve_reference(G, Cm, plans)
    assert want[2].tolist() == [0, 0, 0, 0]
    Gd, Cd = torch.from_numpy(G).cuda(), torch.from_numpy(Cm).cuda()
    for order, at, bad in ((plans + [((1,), 0.0)], 0, 4), ([((1,), 0.0)] + plans, 1, 0)):
        W, b, status = (x.cpu().numpy() for x in R.solve(Gd, Cd, order))
        assert status[bad] == 1 and not W[bad].any() and not b[bad].any()
        assert same_bits(status[at:at + 4], want[2])
        assert same_bits(W[at:at + 4], want[0]), np.abs(W[at:at + 4] - want[0]).max()
        assert same_bits(b[at:at + 4], want[1]), np.abs(b[at:at + 4] - want[1]).max()
    assert R.solve(Gd, Cd, [])[0].shape == (0, 16, 512)


# ---------------------------------------------------------------------------------------------------------------------------
# behind the decoders
# ---------------------------------------------------------------------------------------------------------------------------
def cued(seed=7, reps=3, block=620, gap=90):
    """raw (n, 12) on the GPU and labels (n,): `reps` repetitions of the classes IDS in order, `block` samples each (30 windows)
    with unlabelled gaps between them; noise whose channel amplitudes follow the cue"""
    rng = np.random.default_rng(seed)
    amp = {c: np.random.default_rng([21, c]).uniform(0.4, 3.0, 12) for c in IDS}
    amp[-1] = np.ones(12)
    labels = [np.full(gap, -1)]
    for _ in range(reps):
        for c in IDS:
            labels += [np.full(block, c), np.full(gap, -1)]
    labels = np.concatenate(labels).astype(np.int64)
    raw = (rng.standard_normal((labels.shape[0], 12)) * np.stack([amp[int(c)] for c in labels]) * 2e-3).astype(F)
    return torch.from_numpy(raw).cuda(), labels


@pytest.fixture(scope="module")
def recording():
    raw, labels = cued()
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    w = preprocess_segments(raw[None], keep=20 * np.arange(256))[0]
    return raw, labels, (w.mean(0), w.std(0))


@pytest.mark.parametrize("adapt", [None, 0.0])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_apply_is_the_embedding_of_a_push_with_the_projection_installed(engine, recording, dtype, adapt):
    """adapt=0.0: the adaptive form's kernels with statistics that stay where they are, as the tail inputs take them"""
    raw, labels, norm = recording
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, adapt=adapt)
    fit = R.fit_projection(dec, raw, labels, ridge=[1e-2, 1.0])
    assert fit.status.tolist() == [0, 0] and fit.dtype == dtype and sum(fit.counts.values()) == int((window_labels(labels) >= 0).sum())
    model = [t.clone() for t in dec.projection()]
    z = fit.apply(dec, raw)
    m = windows_before(raw.shape[0], 0)
    assert tuple(z.shape) == (2, m, 16)
    for index in (0, 1):
        fit.install(dec, index)
        assert torch.equal(dec.projection()[1], fit.b[index])
        for windows in (1, 16, 17, 25):
            dec.reset()
            embs = [dec.push(raw[s:s + 20 * windows], return_embeddings=True)[-1] for s in range(0, raw.shape[0], 20 * windows)]
            assert torch.equal(torch.cat(embs), z[index]), (index, windows)
        dec.refresh()                                          # keeps the user's projection
        dec.reset()
        assert torch.equal(dec.push(raw[:2000], return_embeddings=True)[-1], z[index][:windows_before(2000, 0)])
    dec.reset_projection()
    assert all(torch.equal(a, b) for a, b in zip(dec.projection(), model))


@pytest.mark.parametrize("dtype,adapt", [("f32", None), ("bf16", 0.01)])
def test_fit_and_pick_equal_the_definitions_and_leave_the_decoder_alone(engine, recording, dtype, adapt):
    raw, labels, norm = recording
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, vote=9, adapt=adapt)
    dec.push(raw[:777])                                        # a stream in mid-flight with a filled vote ring
    expected = window_labels(labels)
    m = int(expected.shape[0])
    before = dec.ws.clone(), dec.n_seen, [t.clone() for t in dec.projection()], [t.clone() for t in dec.class_table()]
    ridges = [1e-2, 1.0]
    out = R.pick_ridge(dec, raw, expected, ridges)
    rep, n_rep = H.repetitions(expected)
    assert n_rep == 3
    fit = R.fit_projection(dec, raw, labels, rep=(rep, n_rep), plans=out["readout"].plans)
    u = dec._recording_tail_inputs(None, raw, np.arange(m))
    after = dec.ws.clone(), dec.n_seen, dec.projection(), dec.class_table()
    n_state = H._state_bytes(dec, False)                       # stream state, vote ring, the adaptive form's statistics
    assert torch.equal(before[0][:n_state], after[0][:n_state])
    assert before[1] == after[1] == 777
    assert all(torch.equal(a, b) for a, b in zip(before[2], after[2])) and all(torch.equal(a, b) for a, b in zip(before[3], after[3]))
    # ---- the fit against the definition on the decoder's own tail inputs
    table = dec.class_table()[0].cpu().numpy()
    slots = np.where(expected >= 0, np.searchsorted(IDS, np.maximum(expected, 0)), -1)
    want = R.fit_reference(u, slots, R.unit_targets(table), out["readout"].plans, groups=np.where(slots >= 0, rep, -1), n_groups=3)
    assert want["status"].tolist() == [0] * 6 == fit.status.tolist() == out["readout"].status.tolist()
    for got in (fit, out["readout"]):
        assert same_bits(got.W.cpu().numpy(), want["W"]) and same_bits(got.b.cpu().numpy(), want["b"])
    assert fit.counts == {c: int((expected == c).sum()) for c in IDS}
    # ---- the tables against the definitions (the baseline as pick_ridge embeds it: a fresh stream from the current statistics)
    emb0 = H.embed_recording(dec, raw)
    # (f32: through apply_reference, which equals the device in every bit; bf16: the definition's W and b through the device's
    # apply, since the inner order of the bf16 matrix instruction is not reproduced on the host)
    z = None if dtype == "f32" else R.apply(u, want["W"], want["b"])
    ref = R.pick_ridge_reference(u, expected, IDS, table, emb0.cpu().numpy(), ridges, vote=9, dtype=dtype, z=z)
    if dtype == "f32":
        assert same_bits(R.apply_reference(u, want["W"], want["b"]), out["readout"].apply(u).cpu().numpy())
    print("raw", out["raw_hit"], ref["raw_hit"], "voted", out["voted_hit"], ref["voted_hit"], "baseline", out["baseline"], ref["baseline"])
    for key in ("raw_hit", "voted_hit", "n_cue"):
        assert same_bits(out[key], ref[key]), key
    assert out["baseline"] == ref["baseline"] and out["best"] == ref["best"] and out["ridge"] == ref["ridge"]
    lg = out["logits"].cpu().numpy()
    assert lg.shape == (m, 4) and np.isfinite(lg).all()


def test_a_stream_of_a_multi_stream_decoder_fits_as_its_own_decoder(engine, recording):
    raw, labels, norm = recording
    multi = MultiStreamDecoder(engine, *norm, 3, vote=9, dtype="f32")
    multi.set_classes(0, classes=[1, 3])
    multi.set_classes(1, classes=IDS)
    single = OnlineDecoder(engine, *norm, classes=IDS, dtype="f32", vote=9)
    a = R.fit_projection(multi, raw, labels, ridge=0.1, stream=1)
    b = R.fit_projection(single, raw, labels, ridge=0.1)
    assert a.status.tolist() == b.status.tolist() == [0]
    assert torch.equal(a.W, b.W) and torch.equal(a.b, b.b) and a.counts == b.counts
    with pytest.raises(CpNativeError, match="share one projection"):
        a.install(multi)
    with pytest.raises(ValueError, match="stream="):
        R.fit_projection(multi, raw, labels)
    with pytest.raises(ValueError, match="does not have"):
        R.fit_projection(multi, raw, labels, stream=0)
    with pytest.raises(ValueError, match="min_windows"):
        R.fit_projection(single, raw, labels, min_windows=1000)
