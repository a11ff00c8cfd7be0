"""Per-stream projections of the multi-stream decoders on the MI355X (contrastiveprosthetics_amd/online.py
`stream_projections=True`, csrc/online_projections.cuh): every stream with a projection of its own against its own
`OnlineDecoder` with the same projection set, every stream without one against the same decoder built without the option --
push, the widest grid, isolation, enrolment, fine-tuning, the closed-form fit, the map sweep, refresh, a gate behind it and
the C entries.  Every comparison is bit for bit: both sides run the same device functions on the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import _lib
from contrastiveprosthetics_amd import readout as R
from contrastiveprosthetics_amd.online import (AdaptiveMultiStreamDecoder, CommandGate, MultiStreamDecoder, OnlineDecoder, rotations,
                                               score_channel_maps, window_labels, windows_emitted)
from test_gpu_online_finetune import _cued, _engine, _norm, _train_steps

pytestmark = pytest.mark.gpu

IDS = [2, 5, 9, 17, 23, 30]
ALPHA = 0.02
FORMS = pytest.mark.parametrize("dtype,adaptive", [("f32", False), ("bf16", False), ("f32", True), ("bf16", True)])


@pytest.fixture(scope="module")
def engine():
    return _engine()


@pytest.fixture(scope="module")
def cued():
    """six cue blocks of 50..55 windows each: about 315 labelled windows"""
    raw, labels = _cued(31, IDS, lo=1000, hi=1100)
    assert 280 <= int((window_labels(labels, 0) >= 0).sum()) <= 340
    return raw, labels


@pytest.fixture(scope="module")
def norm(cued):
    return _norm(cued)


def _multi(engine, norm, S, dtype, adaptive, on, **kw):
    kw = dict(kw, dtype=dtype, stream_projections=on) if on is not None else dict(kw, dtype=dtype)
    m = AdaptiveMultiStreamDecoder(engine, *norm, S, ALPHA, **kw) if adaptive else MultiStreamDecoder(engine, *norm, S, **kw)
    for s in range(S):
        m.set_classes(s, IDS)
    return m


def _single(engine, norm, dtype, adaptive, proj=None, **kw):
    d = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, adapt=ALPHA if adaptive else None, **kw)
    if proj is not None:
        d.set_projection(*proj)
    return d


def _two_projections(dec):
    """A and B: the decoder's own projection, negated for A (the class it answers with becomes the least likely one, so pred
    and voted move and not only the logits), plus two different perturbations"""
    W0, b0 = dec.projection()
    g = torch.Generator().manual_seed(5)
    out = []
    for sign in (-1.0, 1.0):
        dW = torch.randn(16, 512, generator=g).cuda() * (0.5 * float(W0.abs().max()))
        db = torch.randn(16, generator=g).cuda() * 0.1
        out.append(((sign * W0 + dW).contiguous(), (sign * b0 + db).contiguous()))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _samples_for(seen: int, m: int) -> int:
    """the fewest samples after which a stream that has seen `seen` emits m more windows"""
    n = 0
    while windows_emitted(seen, n, 0) < m:
        n += 1
    return n


ALL = dict(return_logits=True, return_windows=True, return_embeddings=True)


# ---------------------------------------------------------------------------------------------------------------- 1
@FORMS
def test_push_every_stream_equals_its_own_decoder(engine, cued, norm, dtype, adaptive):
    raw, _ = cued
    S = 4
    on, unset, off = (_multi(engine, norm, S, dtype, adaptive, x) for x in (True, True, False))
    assert on.stream_projections and not off.stream_projections and type(on)._shared_projection
    plain = _single(engine, norm, dtype, adaptive)
    A, B = _two_projections(plain)
    assert not torch.equal(A[0], B[0])
    own = {0: A, 2: B}
    singles = [_single(engine, norm, dtype, adaptive, own.get(s)) for s in range(S)]
    on.set_projection(0, *A)
    on.set_projection(2, *B)
    on.set_projection(3, *B)
    on.reset_projection(3)
    assert [on.has_projection(s) for s in range(S)] == [True, False, True, False]
    assert not any(unset.has_projection(s) or off.has_projection(s) for s in range(S))
    seen = [0] * S
    for windows in ((1, 16, 17, 0), (25, 0, 3, 1), (15, 1, 0, 16)):
        chunks = []
        for s, m in enumerate(windows):
            n = _samples_for(seen[s], m)
            chunks.append(raw[1500 * s + seen[s]:1500 * s + seen[s] + n] if n else None)
            seen[s] += n
        got, ref_off, got_unset = on.push(chunks, **ALL), off.push(chunks, **ALL), unset.push(chunks, **ALL)
        for s, m in enumerate(windows):
            assert got[s][0].shape == (m,) and len(got[s]) == 5
            want = singles[s].push(chunks[s], **ALL) if chunks[s] is not None else None
            if want is not None:
                assert _same(got[s], want), (windows, s)
            assert _same(got_unset[s], ref_off[s]), (windows, s)
            if s in (1, 3):
                assert _same(got[s], ref_off[s]), (windows, s)
            elif m:
                assert not torch.equal(got[s][2], ref_off[s][2]), (windows, s)
    # A and B decode the same raw differently, and neither as the model's projection does: a swapped slot cannot pass
    probe = raw[:_samples_for(0, 17)]
    logits = []
    for d in (singles[0], singles[2], plain):
        d.reset()
        logits.append(d.push(probe, return_logits=True)[2])
    assert not torch.equal(logits[0], logits[1]) and not torch.equal(logits[0], logits[2]) and not torch.equal(logits[1], logits[2])


# ---------------------------------------------------------------------------------------------------------------- 2
@FORMS
def test_the_widest_grid_256_streams(engine, cued, norm, dtype, adaptive):
    raw, _ = cued
    S, m = 256, 17
    multi = _multi(engine, norm, S, dtype, adaptive, True, max_windows_per_push=32, max_rows=S * m)
    plain = _single(engine, norm, dtype, adaptive)
    A, B = _two_projections(plain)
    kinds = (None, A, B)
    for s in range(S):
        if kinds[s % 3] is not None:
            multi.set_projection(s, *kinds[s % 3])
    chunk = raw[:_samples_for(0, m)]
    want = [_single(engine, norm, dtype, adaptive, p).push(chunk, **ALL) for p in kinds]
    assert not torch.equal(want[1][2], want[2][2]) and not torch.equal(want[0][2], want[1][2])
    got = multi.push([chunk] * S, **ALL)
    for s in range(S):
        assert got[s][0].shape == (m,) and _same(got[s], want[s % 3]), s


# ---------------------------------------------------------------------------------------------------------------- 3
@FORMS
def test_a_set_touches_its_slot_alone(engine, norm, dtype, adaptive):
    S = 4
    multi = _multi(engine, norm, S, dtype, adaptive, True)
    single = _single(engine, norm, dtype, adaptive)
    A, B = _two_projections(single)
    multi.set_projection(0, *B)
    shared = multi._projection_read(1)
    assert _same(shared, single.projection())
    torch.cuda.synchronize()
    ws, before = multi.ws.clone(), [multi.projection(s) for s in range(S)]
    multi.set_projection(2, *A)
    single.set_projection(*A)
    torch.cuda.synchronize()
    assert torch.equal(multi.ws, ws)
    for s in (0, 1, 3):
        assert _same(multi.projection(s), before[s]), s
    assert _same(multi.projection(1), shared)
    got = multi.projection(2)
    assert _same(got, single.projection())                     # the rounding of W to the compute dtype
    assert torch.equal(got[1], A[1]) and (dtype == "bf16") == (not torch.equal(got[0], A[0]))
    flag = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    W, b = torch.empty(16, 512, device="cuda"), torch.empty(16, device="cuda")
    for s in range(S):
        rc = multi.lib.cp_online_projections_get(*multi._slot_args(s), W.data_ptr(), b.data_ptr(), flag[s:].data_ptr(), multi._stream())
        assert rc == 0, multi.lib.cp_last_error()
    assert flag.tolist() == [1, 0, 1, 0]
    multi.reset_projection()
    assert not any(multi.has_projection(s) for s in range(S)) and _same(multi.projection(2), shared)
    assert torch.equal(multi.ws, ws)


# ---------------------------------------------------------------------------------------------------------------- 4
@FORMS
def test_enrolment_uses_the_streams_own_projection(engine, cued, norm, dtype, adaptive):
    raw, labels = cued
    multi, off = _multi(engine, norm, 3, dtype, adaptive, True), _multi(engine, norm, 3, dtype, adaptive, False)
    plain = _single(engine, norm, dtype, adaptive)
    A, _ = _two_projections(plain)
    single = _single(engine, norm, dtype, adaptive, A)
    multi.set_projection(0, *A)
    counts = multi.enroll(0, raw, labels)
    assert counts == single.enroll(raw, labels) and 280 <= sum(counts.values()) <= 340
    assert _same(multi.class_table(0), single.class_table())
    # a stream without a projection enrols as the decoder without the option does, and not as stream 0
    assert multi.enroll(1, raw, labels) == off.enroll(1, raw, labels)
    assert _same(multi.class_table(1), off.class_table(1))
    assert not torch.equal(multi.class_table(1)[0], multi.class_table(0)[0])


# ---------------------------------------------------------------------------------------------------------------- 5
@FORMS
def test_finetune_trains_the_streams_own_head(engine, cued, norm, dtype, adaptive):
    raw, labels = cued
    kw = dict(steps=5, lr=2e-3, lr_rows=2e-2, scale=4.0, min_windows=5, return_loss=True)
    multi, off = _multi(engine, norm, 3, dtype, adaptive, True), _multi(engine, norm, 3, dtype, adaptive, False)
    with pytest.raises(ValueError, match="shared by all streams"):
        off.finetune(0, raw, labels, **dict(kw, train_projection=True))
    plain = _single(engine, norm, dtype, adaptive)
    A, B = _two_projections(plain)
    single = _single(engine, norm, dtype, adaptive, A)
    multi.set_projection(0, *A)
    multi.set_projection(2, *B)
    other = multi.projection(2), multi.class_table(2), multi.projection(1), multi.class_table(1)
    cm, lm = multi.finetune(0, raw, labels, train_projection=True, **kw)
    cs, ls = single.finetune(raw, labels, train_projection=True, **kw)
    assert cm == cs and torch.equal(lm, ls) and float(lm[4]) < float(lm[0])
    assert _same(multi.projection(0), single.projection()) and not torch.equal(multi.projection(0)[0], A[0])
    assert _same(multi.class_table(0), single.class_table())
    now = multi.projection(2), multi.class_table(2), multi.projection(1), multi.class_table(1)
    assert all(_same(a, b) for a, b in zip(other, now)) and not multi.has_projection(1)
    # a stream without a projection starts from the shared one, as its own decoder starts from the model's
    multi.finetune(1, raw, labels, train_projection=True, **kw)
    plain.finetune(raw, labels, train_projection=True, **kw)
    assert multi.has_projection(1) and _same(multi.projection(1), plain.projection())
    chunk = raw[:700]
    out = multi.push([chunk, chunk, None], **ALL)
    assert _same(out[0], single.push(chunk, **ALL)) and _same(out[1], plain.push(chunk, **ALL))


# ---------------------------------------------------------------------------------------------------------------- 6
@FORMS
def test_a_fitted_readout_installs_into_a_stream(engine, cued, norm, dtype, adaptive):
    raw, labels = cued
    multi, off = _multi(engine, norm, 3, dtype, adaptive, True), _multi(engine, norm, 3, dtype, adaptive, False)
    fit = R.fit_projection(multi, raw, labels, ridge=0.1, stream=0)
    assert fit.status.tolist() == [0]
    with pytest.raises(_lib.CpNativeError, match="share one projection"):
        fit.install(off)
    with pytest.raises(_lib.CpNativeError, match="share one projection"):
        fit.install(off, 0, stream=0)
    z = fit.apply(multi, raw, stream=0)[0]
    stats = multi.bn_statistics(0) if adaptive else None
    fit.install(multi, 0, stream=0)
    assert multi.has_projection(0) and torch.equal(multi.projection(0)[1], fit.b[0])
    for windows in (1, 16, 17, 25):
        multi.reset()
        if adaptive:                                           # the tail inputs were taken with the statistics frozen
            multi.set_alpha(0, 0.0)
            assert torch.equal(multi.bn_statistics(0), stats)
        embs = [multi.push([raw[s:s + 20 * windows], None, None], return_embeddings=True)[0][-1]
                for s in range(0, raw.shape[0], 20 * windows)]
        assert torch.equal(torch.cat(embs), z), windows


# ---------------------------------------------------------------------------------------------------------------- 7
@FORMS
def test_the_map_sweep_scores_with_the_streams_own_projection(engine, cued, norm, dtype, adaptive):
    raw, labels = cued
    multi = _multi(engine, norm, 3, dtype, adaptive, True)
    plain = _single(engine, norm, dtype, adaptive)
    A, _ = _two_projections(plain)
    single = _single(engine, norm, dtype, adaptive, A)
    multi.set_projection(0, *A)
    maps = rotations()[:3]
    got = score_channel_maps(multi, raw, labels, maps, stream=0, return_pred=True, per_class=True)
    want = score_channel_maps(single, raw, labels, maps, return_pred=True, per_class=True)
    base = score_channel_maps(multi, raw, labels, maps, stream=1, return_pred=True, per_class=True)
    model = score_channel_maps(plain, raw, labels, maps, return_pred=True, per_class=True)
    for a, b in ((got, want), (base, model)):
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        for x, y in zip(a[0], b[0]):
            assert {k: v for k, v in x.items() if k != "per_class_voted_hits"} == {k: v for k, v in y.items() if k != "per_class_voted_hits"}
            assert np.array_equal(x["per_class_voted_hits"], y["per_class_voted_hits"])
    assert not torch.equal(got[1], base[1])


# ---------------------------------------------------------------------------------------------------------------- 8
@FORMS
def test_refresh_keeps_a_streams_projection(cued, norm, dtype, adaptive):
    raw, _ = cued
    e = _engine()                                              # its own: the weights move
    multi = _multi(e, norm, 3, dtype, adaptive, True)
    plain = _single(e, norm, dtype, adaptive)
    A, _ = _two_projections(plain)
    single = _single(e, norm, dtype, adaptive, A)
    multi.set_projection(0, *A)
    chunk = raw[:600]
    first = multi.push([chunk, chunk, None], **ALL)
    assert _same(first[0], single.push(chunk, **ALL)) and _same(first[1], plain.push(chunk, **ALL))
    mine, shared = multi.projection(0), multi.projection(1)
    _train_steps(e, 1, 99)
    torch.cuda.synchronize()
    for d in (multi, single, plain):
        d.refresh()
    assert _same(multi.projection(0), mine) and _same(multi.projection(0), single.projection())
    assert not torch.equal(multi.projection(1)[0], shared[0]) and _same(multi.projection(1), plain.projection())
    chunk = raw[600:1300]
    out = multi.push([chunk, chunk, None], **ALL)
    assert _same(out[0], single.push(chunk, **ALL)) and _same(out[1], plain.push(chunk, **ALL))


# ---------------------------------------------------------------------------------------------------------------- 9
@FORMS
def test_a_gate_behind_it_with_every_gate_open(engine, cued, norm, dtype, adaptive):
    raw, _ = cued
    multi = _multi(engine, norm, 3, dtype, adaptive, True, vote=9)
    plain = _single(engine, norm, dtype, adaptive)
    A, B = _two_projections(plain)
    multi.set_projection(0, *A)
    multi.set_projection(2, *B)
    singles = [_single(engine, norm, dtype, adaptive, p, vote=9) for p in (A, None, B)]
    gate = CommandGate(multi)
    for lo in (0, 500, 1000):
        chunks = [raw[lo + 100 * s:lo + 100 * s + 500 - 37 * s] for s in range(3)]
        out = gate.push(chunks)
        for s in range(3):
            pred, voted, cmd, acc = out[s][:4]
            assert torch.equal(cmd, voted) and torch.equal(acc, pred) and voted.shape[0] > 0
            want = singles[s].push(chunks[s])
            assert torch.equal(pred, want[0]) and torch.equal(voted, want[1]), (lo, s)


# ---------------------------------------------------------------------------------------------------------------- 10
@FORMS
def test_the_c_entries_null_bank_and_short_bank(engine, cued, norm, dtype, adaptive):
    raw, _ = cued
    S = 3
    a, b = _multi(engine, norm, S, dtype, adaptive, False), _multi(engine, norm, S, dtype, adaptive, False)
    lib = a.lib
    embed = getattr(lib, a._ENTRY + "_push_embed")
    proj = getattr(lib, a._ENTRY + "_push_proj")
    counts = np.array([_samples_for(0, 17), 0, _samples_for(0, 3)], dtype=np.int32)
    rows = 20
    piece = torch.cat([raw[:counts[0]], raw[3000:3000 + counts[2]]]).contiguous()
    cdev = torch.from_numpy(counts).cuda()

    def outputs():
        return [torch.full((rows,), -7, dtype=torch.int32, device="cuda"), torch.full((rows,), -7, dtype=torch.int32, device="cuda"),
                torch.full((rows, 64), -7.0, device="cuda"), torch.full((rows, 12), -7.0, device="cuda"),
                torch.full((rows, 16), -7.0, device="cuda")]

    def call(fn, dec, out, *bank):
        return fn(*dec._args(), piece.data_ptr(), cdev.data_ptr(), int(piece.shape[0]), rows, dec.mean_std.data_ptr(), None, None,
                  *[t.data_ptr() for t in out], *bank, dec._stream())

    out_a, out_b = outputs(), outputs()
    assert call(embed, a, out_a) == 0, lib.cp_last_error()
    assert call(proj, b, out_b, None, 0) == 0, lib.cp_last_error()
    torch.cuda.synchronize()
    assert _same(out_a, out_b) and torch.equal(a.ws, b.ws)
    assert float(out_a[4].min()) > -7.0
    # a short bank: refused before anything is enqueued
    need = lib.cp_online_projections_bytes(S, a._cfg.dtype)
    bank = torch.zeros(need, dtype=torch.uint8, device="cuda")
    ws = b.ws.clone()
    sentinel = outputs()
    rc = call(proj, b, sentinel, bank.data_ptr(), need - 1)
    assert rc == 10002 and b"_push_proj: bank too small" in lib.cp_last_error()
    torch.cuda.synchronize()
    assert _same(sentinel, outputs()) and torch.equal(b.ws, ws)
    # the whole bank, zeroed: the entry with no slot set is the _push_embed entry in every output
    out_c = outputs()
    a.reset()
    b.reset()
    assert call(embed, a, out_a) == 0 and call(proj, b, out_c, bank.data_ptr(), need) == 0, lib.cp_last_error()
    torch.cuda.synchronize()
    assert _same(out_a, out_c) and not bank.any()
