"""Class enrolment on the MI355X (contrastiveprosthetics_amd/online.py enroll / recording_windows, csrc/online_enroll.cuh):
one-pass windows bit-identical to the offline path and to a push, the order contract of the accumulator, z / |z| as the push
computes it, the per-class means against the engine's eval path, the blend (mix, min_windows, add, refresh), the adaptive
forms (statistics untouched, AdaBN after calibration) and the multi-stream decoders against their single-stream twins."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
IDS = list(range(41))
SHORT = 7                                    # the class whose cue block is too short for min_windows = 25
NEW = 50                                     # a grasp the model was never trained on


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


def _amplitudes(seed=21):
    """per class (and NEW) a pattern of channel amplitudes: the class signal of the synthetic recordings"""
    rng = np.random.default_rng(seed)
    amp = {c: rng.uniform(0.4, 3.0, 12) for c in IDS}
    # the new grasp lies well outside the others: an 11-sample RMS scatters by about 1 / sqrt(22) = 21 % per channel, which
    # blurs the 41 patterns above into each other but not a pattern that is 8 on six channels and 0.2 on the rest
    amp[NEW] = np.where(np.arange(12) < 6, 8.0, 0.2)
    amp[-1] = np.ones(12)
    return amp


def _cued(seed, ids, short=(), lo=540, hi=640):
    """A cued recording: seeded cue blocks over `ids` in a shuffled order with unlabelled gaps between them; the signal is
    noise whose channel amplitudes follow the cue.  Returns raw (n, 12) f32 on the GPU and labels (n,) int64."""
    rng = np.random.default_rng(seed)
    amp = _amplitudes()
    labels = [np.full(int(rng.integers(30, 120)), -1)]
    for c in rng.permutation(ids):
        n = int(rng.integers(180, 220)) if c in short else int(rng.integers(lo, hi))
        labels += [np.full(n, int(c)), np.full(int(rng.integers(30, 120)), -1)]
    labels = np.concatenate(labels).astype(np.int64)
    scale = np.stack([amp[int(c)] for c in labels])
    raw = (rng.standard_normal((labels.shape[0], 12)) * scale * 2e-3).astype(np.float32)
    return torch.from_numpy(raw).cuda(), labels


@pytest.fixture(scope="module")
def cued():
    return _cued(31, IDS, short=(SHORT,))


@pytest.fixture(scope="module")
def norm(cued):
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    w = preprocess_segments(cued[0][None], keep=20 * np.arange(256))[0]
    return w.mean(0), w.std(0)


def _labelled(dec, raw, labels):
    """the labelled windows of a recording and their slots in dec.class_ids, as enroll() forms them"""
    from contrastiveprosthetics_amd.online import recording_windows, window_labels
    wl = window_labels(labels, dec.phase)
    keep = np.nonzero(wl >= 0)[0]
    w = recording_windows(raw, dec.mean_std, dec._b, dec._a, dec.phase)[torch.as_tensor(keep).cuda()].contiguous()
    slots = np.searchsorted(dec.class_ids.numpy(), wl[keep]).astype(np.int32)
    return w, torch.from_numpy(slots).cuda(), keep, wl


def _accumulate(dec, w, slots, cuts, acc=None):
    """cp_online_enroll over the windows cut into calls of the given lengths"""
    lib = dec.lib
    acc = torch.zeros(64, 17, dtype=torch.float64, device="cuda") if acc is None else acc
    fn = lib.cp_online_enroll if dec.adapt is None else lib.cp_online_adapt_enroll
    s = 0
    for n in cuts:
        if n == 0:
            continue
        scratch = torch.empty(lib.cp_online_enroll_scratch_bytes(n, dec._cfg.dtype), dtype=torch.uint8, device="cuda")
        rc = fn(C.byref(dec._cfg), dec.ws.data_ptr(), dec.ws.numel(), w[s:s + n].data_ptr(), n, slots[s:s + n].data_ptr(),
                dec.class_ids.numel(), acc.data_ptr(), scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.cp_last_error()
        s += n
    assert s == w.shape[0]
    torch.cuda.synchronize()
    return acc


def _table_from(dec, acc, prior, mix=1.0, min_windows=25):
    out = torch.empty_like(prior)
    rc = dec.lib.cp_online_enroll_table(acc.data_ptr(), prior.shape[0], prior.data_ptr(), C.c_double(mix), min_windows, out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, dec.lib.cp_last_error()
    return out


def _pieces(total, n):
    return [n] * (total // n) + ([total % n] if total % n else [])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("phase", [0, 13])
def test_recording_windows_equal_the_offline_path_and_a_push(engine, cued, norm, phase):
    from contrastiveprosthetics_amd import OnlineDecoder, recording_windows
    from contrastiveprosthetics_amd.online import _calibration_windows, windows_before
    raw, _ = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, phase=phase)
    w = recording_windows(raw, dec.mean_std, dec._b, dec._a, phase)
    assert w.shape == (windows_before(raw.shape[0], phase), 12) and w.shape[0] > 1024          # several chunks of 256 windows
    assert torch.equal(w, _calibration_windows(raw, dec._b, dec._a, phase, dec.mean_std))
    assert torch.equal(w, dec.push(raw, return_windows=True)[2])
    assert torch.equal(w[:7], recording_windows(raw[:phase + 20 * 6 + 11], dec.mean_std, phase=phase))     # default filter, a short one
    assert recording_windows(raw[:5], dec.mean_std, phase=phase).shape == (0, 12)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_accumulator_depends_on_the_window_sequence_only(engine, cued, norm, dtype):
    from contrastiveprosthetics_amd import OnlineDecoder
    raw, labels = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype)
    w, slots, keep, _ = _labelled(dec, raw, labels)
    N = w.shape[0]
    assert N > 41 * 25
    whole = _accumulate(dec, w, slots, [N])
    counts = np.bincount(slots.cpu().numpy(), minlength=64)
    assert np.array_equal(whole[:, 16].cpu().numpy(), counts.astype(np.float64))
    assert float(whole[41:].abs().max()) == 0.0
    rng = np.random.default_rng(4)
    rnd, s = [], 0
    while s < N:
        rnd.append(int(min(rng.integers(1, 400), N - s)))
        s += rnd[-1]
    for name, cuts in (("1", [1] * N), ("16", _pieces(N, 16)), ("333", _pieces(N, 333)), ("random", rnd)):
        assert torch.equal(_accumulate(dec, w, slots, cuts), whole), name
    # slots outside 0..n_classes-1 are skipped
    odd = slots.clone()
    odd[::3] = -1
    odd[1::3] = 41
    part = _accumulate(dec, w, odd, [N])
    assert torch.equal(part, _accumulate(dec, w[2::3].contiguous(), slots[2::3].contiguous(), [w[2::3].shape[0]]))

    # enroll(A, accumulate=True), then enroll(B): the table of the concatenated (window, label) sequence
    rawB, labB = _cued(32, IDS)
    prior = dec.class_table()[0]
    cA = dec.enroll(raw, labels, accumulate=True)
    assert cA == {i: int(counts[i]) for i in IDS}
    assert torch.equal(dec.class_table()[0], prior)                       # the table is left alone
    cB = dec.enroll(rawB, labB)
    wB, slotsB, _, _ = _labelled(dec, rawB, labB)
    both = _accumulate(dec, torch.cat([w, wB]), torch.cat([slots, slotsB]), [N + wB.shape[0]])
    assert cB == {i: int(both[i, 16]) for i in IDS}
    assert torch.equal(dec.class_table()[0], _table_from(dec, both, prior))
    dec.enroll_reset()
    assert dec.enroll(rawB, labB, accumulate=True) == {i: int(c) for i, c in enumerate(np.bincount(slotsB.cpu().numpy(), minlength=41))}


# ---------------------------------------------------------------------------------------------------------------- 3
def _one_window_per_class(labels_len, phase, seed=9):
    """labels that give exactly one labelled window to each of the 41 classes"""
    rng = np.random.default_rng(seed)
    from contrastiveprosthetics_amd.online import windows_before
    K = windows_before(labels_len, phase)
    ks = np.sort(rng.choice(np.arange(2, K, 3), size=41, replace=False))           # no two spans touch
    lab = np.full(labels_len, -1, dtype=np.int64)
    cls = rng.permutation(41)
    for k, c in zip(ks, cls):
        lab[phase + 20 * k: phase + 20 * k + 11] = c
    return lab, ks, cls


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("adapt", [None, 0.0])
def test_enrolled_windows_meet_their_own_rows_in_a_push(engine, cued, norm, dtype, adapt):
    """A unit vector against itself after two f32 normalisations and a 16-term dot: about 30 roundings of 2**-24 = 1.8e-6;
    1e-5 gives 5x.  It holds in bf16 too: z reaches the tail in f32 in both passes.  (adapt=0.0: the adaptive form with its
    statistics frozen, which is what its enrolment embeds with.)"""
    from contrastiveprosthetics_amd import OnlineDecoder
    from contrastiveprosthetics_amd.online import window_labels
    raw, _ = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, adapt=adapt)
    lab, ks, cls = _one_window_per_class(raw.shape[0], 0)
    wl = window_labels(lab, 0)
    assert (wl >= 0).sum() == 41 and np.array_equal(wl[ks], cls)
    counts = dec.enroll(raw, lab, min_windows=1, mix=1.0)
    assert counts == {i: 1 for i in IDS}
    dec.reset()
    _, _, logits = dec.push(raw, return_logits=True)
    rows = logits[torch.as_tensor(ks).cuda()]
    own = rows[torch.arange(41), torch.as_tensor(cls).cuda()]
    print(f"{dtype} adapt={adapt}: max |1 - own logit| {float((own - 1).abs().max()):.3e}")
    assert torch.equal(own, rows.max(dim=1).values)
    assert float((own - 1).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 4
def _engine_zn(engine, windows):
    n = windows.shape[0]
    x = torch.zeros((n + 40) // 41 * 41, 12, device=windows.device)          # the encoder takes whole groups of 41 rows
    x[:n] = windows
    z = engine.encoder_forward(x, training=False)[:n].double()
    return z / z.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("dtype,bound", [("f32", 1e-4), ("bf16", 2e-2)])
def test_class_means_against_the_eval_path(engine, cued, norm, dtype, bound):
    """acc[:, :16] / count against the float64 per-class mean of z / |z| from Engine.encoder_forward(training=False).  A mean
    of unit vectors is off by at most what one of them is, so the bounds are those of test_against_the_eval_path for the same
    two paths: 1e-4 (f32 decoder), 2e-2 (bf16 decoder against the f32 path).  The un-normalised means are compared: where a
    class's directions cancel, S / |S| would amplify the error."""
    from contrastiveprosthetics_amd import OnlineDecoder
    raw, labels = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype)
    w, slots, _, _ = _labelled(dec, raw, labels)
    acc = _accumulate(dec, w, slots, [w.shape[0]])
    zn = _engine_zn(engine, w)
    ref = torch.zeros(41, 16, dtype=torch.float64, device="cuda").index_add_(0, slots.long(), zn)
    cnt = torch.bincount(slots.long(), minlength=41).double()
    assert torch.equal(acc[:41, 16], cnt) and int(cnt.min()) >= 5
    dev = float((acc[:41, :16] / cnt[:, None] - ref / cnt[:, None]).abs().max())
    print(f"{dtype} enrolment vs encoder_forward(eval): max |mean z^ diff| {dev:.3e} over {w.shape[0]} windows, "
          f"shortest mean {float((ref / cnt[:, None]).norm(dim=1).min()):.3f}")
    assert dev <= bound


# ---------------------------------------------------------------------------------------------------------------- 5
def test_mix_min_windows_add_and_refresh(engine, cued, norm):
    from contrastiveprosthetics_amd import OnlineDecoder
    from contrastiveprosthetics_amd.online import window_labels
    raw, labels = cued
    probe = raw[:6000]
    dec = OnlineDecoder(engine, *norm, classes=IDS)
    before = dec.push(probe, return_logits=True)
    prior, ids = dec.class_table()
    # mix = 0: the table, and with it every logit, is what it was
    counts = dec.enroll(raw, labels, mix=0.0)
    assert counts[SHORT] < 25 <= min(c for i, c in counts.items() if i != SHORT)
    assert torch.equal(dec.class_table()[0], prior)
    dec.reset()
    after = dec.push(probe, return_logits=True)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    # mix = 1: the prototypes; a table stored and put back decodes bit for bit the same
    dec.enroll_reset()
    dec.enroll(raw, labels, mix=1.0)
    rows, ids2 = dec.class_table()
    assert torch.equal(ids2, ids) and dec._source[2] is not None
    assert torch.equal(rows[SHORT], prior[SHORT])                         # below min_windows: the prior row
    others = [i for i in IDS if i != SHORT]
    assert not any(torch.equal(rows[i], prior[i]) for i in others)
    acc = _accumulate(dec, *_labelled(dec, raw, labels)[:2], [int((window_labels(labels, 0) >= 0).sum())])
    unit = acc[:41, :16] / acc[:41, :16].norm(dim=1, keepdim=True)
    cos = ((rows.double() / rows.double().norm(dim=1, keepdim=True)) * unit).sum(1)
    assert float((1 - cos[others]).abs().max()) <= 1e-6                   # f32 rows of a float64 direction
    twin = OnlineDecoder(engine, *norm)
    twin.set_classes(table=rows, ids=ids2)
    dec.reset()
    a, b = dec.push(probe, return_logits=True), twin.push(probe, return_logits=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[2], before[2])
    # a half-way blend lies between the two
    mid = OnlineDecoder(engine, *norm, classes=IDS)
    mid.enroll(raw, labels, mix=0.5)
    m = mid.class_table()[0].double()
    want = 0.5 * prior.double() / prior.double().norm(dim=1, keepdim=True) + 0.5 * unit
    mcos = ((m / m.norm(dim=1, keepdim=True)) * (want / want.norm(dim=1, keepdim=True))).sum(1)
    assert float((1 - mcos[others]).abs().max()) <= 1e-6 and torch.equal(mid.class_table()[0][SHORT], prior[SHORT])
    # refresh() keeps an enrolled table
    dec.refresh()
    assert torch.equal(dec.class_table()[0], rows)
    dec.reset()
    assert all(torch.equal(x, y) for x, y in zip(dec.push(probe, return_logits=True), a))
    # an id the decoder does not have
    rawN, labN = _cued(33, [NEW, 3, 12])
    with pytest.raises(ValueError, match="does not have"):
        dec.enroll(rawN, labN)
    assert torch.equal(dec.class_table()[0], rows)                        # nothing was enqueued
    with pytest.raises(ValueError, match="fewer than min_windows"):
        dec.enroll(rawN, labN, add=True, min_windows=40)
    counts = dec.enroll(rawN, labN, add=True)
    rows42, ids42 = dec.class_table()
    assert ids42.tolist() == IDS + [NEW] and rows42.shape == (42, 16) and counts[NEW] >= 25
    dec.reset()
    pred = dec.push(rawN)[0].cpu().numpy()
    wl = window_labels(labN, 0)
    own = pred[wl == NEW]
    share = float((own == NEW).mean())
    print(f"add=True: {share:.3f} of the new grasp's {own.size} windows are predicted as it (chance 1/42)")
    # the row is the mean direction of exactly these windows; with a class signal they lie nearer to it than to the 41 rows
    # of other cues: most of them must come back as NEW
    assert share >= 0.9
    full = OnlineDecoder(engine, *norm)
    full.set_classes(table=torch.randn(64, 16, generator=torch.Generator().manual_seed(1)), ids=list(range(64)))
    with pytest.raises(ValueError, match="at most 64"):
        full.enroll(rawN, np.where(labN == NEW, 70, labN), add=True)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_adaptive_forms(engine, ada, cued, norm):
    from contrastiveprosthetics_amd import OnlineDecoder, _lib
    raw, labels = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, adapt=0.05)
    dec.push(raw[:3000])                                                  # the statistics have moved off the running ones
    stats = dec.bn_statistics()
    prior = dec.class_table()[0]
    counts = dec.enroll(raw, labels)
    assert torch.equal(dec.bn_statistics(), stats)                        # enrolment never moves statistics
    assert counts[SHORT] < 25 and not torch.equal(dec.class_table()[0], prior)
    # the frozen statistics are the ones enrolment embeds with: a decoder frozen at them gets the same accumulator
    w, slots, _, _ = _labelled(dec, raw, labels)
    a1 = _accumulate(dec, w, slots, [w.shape[0]])
    assert torch.equal(a1, _accumulate(dec, w, slots, _pieces(w.shape[0], 100)))
    assert torch.equal(dec.bn_statistics(), stats)

    d = OnlineDecoder(ada, *norm, classes=IDS, adapt=0.0)
    with pytest.raises(_lib.CpNativeError, match="calibrate"):
        d.enroll(raw, labels)
    d.calibrate(raw[:8000])
    stats = d.bn_statistics()
    prior = d.class_table()[0]
    counts = d.enroll(raw, labels)
    assert torch.equal(d.bn_statistics(), stats) and not torch.equal(d.class_table()[0], prior)
    assert sum(counts.values()) == int((_labelled(d, raw, labels)[3] >= 0).sum())


# ---------------------------------------------------------------------------------------------------------------- 7
def _push_all(multi, recs, lo, hi, idle=()):
    chunks = [None if s in idle else recs[s][lo:hi] for s in range(multi.n_streams)]
    return multi.push(chunks, return_logits=True, return_windows=True)


def _same(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y), what


@pytest.mark.parametrize("adaptive", [False, True])
def test_multi_stream_enrolment_matches_the_single_stream_decoder(engine, cued, norm, adaptive):
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, MultiStreamDecoder, OnlineDecoder
    raw, labels = cued
    S, s_en, alpha = 5, 2, 0.05
    rng = np.random.default_rng(17)
    recs = [torch.from_numpy((rng.standard_normal((3000, 12)) * (1 + 0.2 * i) * 2e-3).astype(np.float32)).cuda() for i in range(S)]
    subsets = [IDS, [3, 9, 27], IDS, list(range(0, 41, 2)), [1, 2]]

    def build():
        m = AdaptiveMultiStreamDecoder(engine, *norm, S, alpha) if adaptive else MultiStreamDecoder(engine, *norm, S)
        for s in range(S):
            m.set_classes(s, subsets[s])
        return m

    multi, twin = build(), build()                                        # twin never enrols
    single = OnlineDecoder(engine, *norm, classes=subsets[s_en], adapt=alpha if adaptive else None)
    idle = (1, 4)
    for m in (multi, twin):
        _push_all(m, recs, 0, 900, idle)
    single.push(recs[s_en][:900])
    stats = [multi.bn_statistics(s) for s in range(S)] if adaptive else None
    cm = multi.enroll(s_en, raw, labels)
    cs = single.enroll(raw, labels)
    assert cm == cs
    _same(multi.class_table(s_en), single.class_table(), "table")
    assert not torch.equal(multi.class_table(s_en)[0], twin.class_table(s_en)[0])
    for s in range(S):
        if s != s_en:
            _same(multi.class_table(s), twin.class_table(s), ("table", s))
        if adaptive:
            assert torch.equal(multi.bn_statistics(s), stats[s]), s
    out, ref = _push_all(multi, recs, 900, 2100, idle=(4,)), _push_all(twin, recs, 900, 2100, idle=(4,))
    r = single.push(recs[s_en][900:2100], return_logits=True, return_windows=True)
    for s in range(S):
        if s == s_en:
            _same(out[s], r, "enrolled stream")
            assert not torch.equal(out[s][2], ref[s][2])
        else:
            _same(out[s], ref[s], ("other stream", s))
    if adaptive:
        assert torch.equal(multi.bn_statistics(s_en), single.bn_statistics())
        for s in range(S):
            assert torch.equal(multi.bn_statistics(s), twin.bn_statistics(s)), s
