"""Head fine-tuning on the MI355X (contrastiveprosthetics_amd/online.py finetune / projection, csrc/online_finetune.cuh): the
step-0 loss pinned to the logits of a push, one and five steps against the float64 reference at the kernel's rounding points,
determinism and the cut of steps into calls, untrained tensors bit-identical, the stored head put back, refresh, the adaptive
form's statistics, the multi-stream decoders against their single-stream twin, and the tail inputs under any cut."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from finetune_problem import synthetic_problem  # noqa: E402  (tests/finetune_problem.py)

pytestmark = pytest.mark.gpu

PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
IDS = list(range(41))
NS = (1, 15, 16, 17, 63, 64, 65, 130)        # one tile and one chunk (64 rows), each +-1, and three chunks
KS = (2, 41, 64)

# Measured on the MI355X over NS x KS (class K-1 without windows), printed by the tests below; each bound is 4 x the
# largest deviation seen.
#   step-0 loss against the float64 cross-entropy of the push's logits, relative:   f32 5.191e-8, bf16 5.816e-8
#   dW, db, dE and the masters after 1 and 5 steps against finetune_reference, relative to the tensor's largest entry:
#                                                       f32 7.21e-7 (E after 5 steps), bf16 2.11e-6 (W after 5 steps)
#   the same against the reference without the z^ (z^ . dz^) term: 3.3e-2 at the least (dW and db, both dtypes)
LOSS_BOUND = {"f32": 4 * 5.191e-8, "bf16": 4 * 5.816e-8}
STEP_BOUND = {"f32": 4 * 7.21e-7, "bf16": 4 * 2.11e-6}


def _train_steps(e, steps, seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(41).repeat(4).cuda()
    for _ in range(steps):
        x = (torch.randn(4 * 41, 12, generator=g) * 1.5 + 0.3).cuda()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(PARAMS)


def _engine():
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=False, dtype="f32", device="cuda:0", seed=3)
    e.init_parameters(3)
    _train_steps(e, 3, 3)
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def engine():
    return _engine()


def _cued(seed, ids, lo=200, hi=260):
    """A cued recording as tests/test_gpu_online_enroll.py builds its own, with shorter cue blocks (9..12 windows each): seeded
    cue blocks over `ids` in a shuffled order with unlabelled gaps, noise whose channel amplitudes follow the cue."""
    rng = np.random.default_rng(seed)
    amp = {c: np.random.default_rng([21, c]).uniform(0.4, 3.0, 12) for c in ids}
    amp[-1] = np.ones(12)
    labels = [np.full(int(rng.integers(30, 120)), -1)]
    for c in rng.permutation(ids):
        labels += [np.full(int(rng.integers(lo, hi)), int(c)), np.full(int(rng.integers(30, 120)), -1)]
    labels = np.concatenate(labels).astype(np.int64)
    scale = np.stack([amp[int(c)] for c in labels])
    raw = (rng.standard_normal((labels.shape[0], 12)) * scale * 2e-3).astype(np.float32)
    return torch.from_numpy(raw).cuda(), labels


@pytest.fixture(scope="module")
def cued():
    return _cued(31, IDS)


def _norm(cued):
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    w = preprocess_segments(cued[0][None], keep=20 * np.arange(256))[0]
    return w.mean(0), w.std(0)


@pytest.fixture(scope="module")
def norm(cued):
    return _norm(cued)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cfg(dtype):
    from contrastiveprosthetics_amd import online
    b, a = online._filter(None, None)
    return online._config(dtype, 256, 25, 0, b, a)


class _Run:
    """cp_online_finetune_init on device copies of (u, W, b, E, slots), then steps in the calls asked for"""

    def __init__(self, lib, dtype, u, W, b, E, slots, balanced=True):
        self.lib, self.cfg = lib, _cfg(dtype)
        dev = lambda x, dt: torch.as_tensor(np.asarray(x)).to(dt).cuda().contiguous() if not isinstance(x, torch.Tensor) else x.to(dt).contiguous()
        self.u = dev(u, torch.float32 if dtype == "f32" else torch.bfloat16)
        self.W, self.b, self.E = dev(W, torch.float32), dev(b, torch.float32), dev(E, torch.float32)
        self.slots = dev(slots, torch.int32)
        self.n, self.k = int(self.u.shape[0]), int(self.E.shape[0])
        # (zeroed, so that two states can be compared whole: the padding between its blocks is never written)
        self.state = torch.zeros(lib.cp_online_finetune_state_bytes(self.n, self.k), dtype=torch.uint8, device="cuda")
        rc = lib.cp_online_finetune_init(self.state.data_ptr(), self.state.numel(), self.cfg.dtype, self.W.data_ptr(), self.b.data_ptr(),
                                         self.E.data_ptr(), self.slots.data_ptr(), self.n, self.k, int(balanced), _stream())
        assert rc == 0, lib.cp_last_error()

    def steps(self, n_steps, lr=1e-3, lr_rows=1e-2, scale=4.0, anchor=0.0, flags=3):
        loss = torch.full((max(n_steps, 1),), float("nan"), dtype=torch.float64, device="cuda")
        rc = self.lib.cp_online_finetune_steps(C.byref(self.cfg), self.state.data_ptr(), self.state.numel(), self.u.data_ptr(), self.n,
                                               self.k, n_steps, lr, lr_rows, scale, anchor, flags, loss.data_ptr(), _stream())
        assert rc == 0, self.lib.cp_last_error()
        return loss[:n_steps]

    def read(self):
        W, b, E = torch.empty(16, 512, device="cuda"), torch.empty(16, device="cuda"), torch.empty(self.k, 16, device="cuda")
        grad = torch.empty(8208 + 16 * self.k, dtype=torch.float64, device="cuda")
        rc = self.lib.cp_online_finetune_read(self.state.data_ptr(), self.state.numel(), self.n, self.k, W.data_ptr(), b.data_ptr(),
                                              E.data_ptr(), grad.data_ptr(), _stream())
        assert rc == 0, self.lib.cp_last_error()
        torch.cuda.synchronize()
        g = grad.cpu().numpy()
        return dict(W=W.cpu().double().numpy(), b=b.cpu().double().numpy(), E=E.cpu().double().numpy(),
                    grad=(g[:8192].reshape(16, 512), g[8192:8208], g[8208:].reshape(self.k, 16)))


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_step_zero_loss_is_the_cross_entropy_of_the_push_logits(engine, cued, norm, dtype):
    """The forward of a step is the forward of a push: W_T u + b through the same tile code, z^ and E^ normalised and the
    cosines summed as the tail does.  What is left between the device's loss and the float64 cross-entropy of the logits a
    push returns is the softmax's f32 arithmetic (expf, logf, a 64-lane sum, one division)."""
    from contrastiveprosthetics_amd import OnlineDecoder
    from contrastiveprosthetics_amd.finetune import class_weights
    from contrastiveprosthetics_amd.online import recording_windows, window_labels
    raw, labels = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype)
    wl = window_labels(labels, 0)
    keep = np.nonzero(wl >= 0)[0][:max(NS)]
    assert keep.size == max(NS)
    W, b = dec.projection()
    worst = 0.0
    for k in KS:
        E = torch.randn(k, 16, generator=torch.Generator().manual_seed(k)).cuda()
        dec.set_classes(table=E, ids=list(range(k)))
        dec.reset()
        logits = dec.push(raw, return_logits=True)[2][torch.as_tensor(keep).cuda()].double().cpu().numpy()
        w = recording_windows(raw, dec.mean_std, dec._b, dec._a, 0)[torch.as_tensor(keep).cuda()].contiguous()
        u = torch.empty(w.shape[0], 512, dtype=torch.float32 if dtype == "f32" else torch.bfloat16, device="cuda")
        dec._tail_inputs_call(None, w.data_ptr(), int(w.shape[0]), u.data_ptr(), *_scratch(dec, w.shape[0]))
        slots = (wl[keep] % max(k - 1, 1)).astype(np.int32)      # class k-1 without windows
        for n in NS:
            for balanced in (True, False):
                run = _Run(dec.lib, dtype, u[:n], W, b, E, slots[:n], balanced)
                got = float(run.steps(1, flags=0, scale=1.0)[0])
                wi = class_weights(slots[:n], k, balanced, f32=True)
                l = logits[:n]
                nll = np.log(np.exp(l - l.max(1, keepdims=True)).sum(1)) + l.max(1) - l[np.arange(n), slots[:n]]
                want = float((wi * nll).sum())
                worst = max(worst, abs(got - want) / abs(want))
    print(f"{dtype}: step-0 loss vs float64 cross-entropy of the push logits, largest relative deviation {worst:.3e} "
          f"(bound {LOSS_BOUND[dtype]:.3e})")
    assert worst <= LOSS_BOUND[dtype]


def _scratch(dec, n):
    s = torch.empty(dec.lib.cp_online_enroll_scratch_bytes(int(n), dec._cfg.dtype), dtype=torch.uint8, device="cuda")
    dec._scratch_keep = s
    return s.data_ptr(), s.numel()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_and_five_steps_against_the_reference(dtype):
    """dW, db, dE of the first step and the masters after 1 and after 5 steps against finetune_reference with u and W_T as
    stored and z^, E^, w_i, masters and moments in f32.  The same comparison against a reference whose normalisation backward
    lacks the z^ (z^ . dz^) term must miss the bound by 100 x: a bound that could hide that mistake is no bound."""
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.finetune import finetune_reference, round_bf16
    lib = _lib.load()
    hyper = dict(lr=1e-3, lr_rows=1e-2, scale=4.0, anchor=0.05)
    worst, wrong_least = {}, {}
    for n in NS:
        for k in KS:
            q = synthetic_problem(n, k, seed=11, bf16=dtype == "bf16")
            run = _Run(lib, dtype, q["u"], q["W"], q["b"], q["E"], q["slots"])
            run.steps(1, **hyper)
            one = run.read()
            run.steps(4, **hyper)
            five = run.read()
            kw = dict(steps=5, round_w=round_bf16 if dtype == "bf16" else None, f32_points=True, **hyper)
            ref = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], **kw)
            first = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], **dict(kw, steps=1))
            bad = finetune_reference(q["u"], q["W"], q["b"], q["E"], q["slots"], **dict(kw, steps=1, normalisation_backward=False))
            pairs = {"dW": (one["grad"][0], first["grad"][0]), "db": (one["grad"][1], first["grad"][1]),
                     "dE": (one["grad"][2], first["grad"][2])}
            for i, name in enumerate(("W", "b", "E")):
                pairs[name + "1"] = (one[name], ref["trace"][0][i])
                pairs[name + "5"] = (five[name], ref["trace"][4][i])
            for name, (got, want) in pairs.items():
                worst[name] = max(worst.get(name, 0.0), _rel(got, want))
            for i, name in enumerate(("dW", "db")):
                wrong_least[name] = min(wrong_least.get(name, np.inf), _rel(one["grad"][i], bad["grad"][i]))
    print(f"{dtype}: largest deviation from the reference relative to each tensor's largest entry over {len(NS) * len(KS)} shapes: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {STEP_BOUND[dtype]:.2e}); against the reference without "
          + "the normalisation term, smallest: " + ", ".join(f"{k} {v:.2e}" for k, v in wrong_least.items()))
    assert max(worst.values()) <= STEP_BOUND[dtype]
    assert min(wrong_least.values()) >= 100 * STEP_BOUND[dtype]


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_runs_repeat_and_do_not_depend_on_the_cut_into_calls(dtype):
    from contrastiveprosthetics_amd import _lib
    lib = _lib.load()
    q = synthetic_problem(130, 41, seed=2, bf16=dtype == "bf16")

    def run(cuts):
        r = _Run(lib, dtype, q["u"], q["W"], q["b"], q["E"], q["slots"])
        loss = torch.cat([r.steps(c, anchor=0.01) for c in cuts])
        out = r.read()
        return r.state.clone(), loss, out

    a, b, c = run([6]), run([6]), run([2, 4])
    for other, what in ((b, "a second run"), (c, "2 + 4 steps")):
        assert torch.equal(a[1], other[1]), (what, "loss series")
        for name in ("W", "b", "E"):
            assert np.array_equal(a[2][name], other[2][name]), (what, name)
        assert all(np.array_equal(x, y) for x, y in zip(a[2]["grad"], other[2]["grad"])), (what, "gradient")
        assert torch.equal(a[0], other[0]), (what, "state: moments, step count, slabs")
    assert float(a[1][5]) < float(a[1][0])


# ---------------------------------------------------------------------------------------------------------------- 4
def _probe(dec, raw):
    dec.reset()
    return dec.push(raw, return_logits=True)


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_untrained_parts_round_trip_and_refresh(engine, cued, norm, dtype):
    from contrastiveprosthetics_amd import OnlineDecoder
    raw, labels = cued
    kw = dict(steps=8, lr=2e-3, lr_rows=2e-2, scale=4.0, min_windows=5)
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype)
    model_out = _probe(dec, raw)
    W0, b0 = dec.projection()
    E0, ids0 = dec.class_table()
    # steps = 0 changes nothing
    dec.push(raw[4000:4600])                                     # a vote ring that is not empty
    counts = dec.finetune(raw, labels, **dict(kw, steps=0))
    assert sum(counts.values()) > 41 * 5 and min(counts.values()) >= 5
    assert _same(dec.projection(), (W0, b0)) and _same(dec.class_table(), (E0, ids0))
    assert _same(_probe(dec, raw), model_out)
    # rows only: the projection is bit-identical, the table moved
    c2, loss = dec.finetune(raw, labels, train_projection=False, return_loss=True, **kw)
    assert c2 == counts and loss.shape == (8,) and float(loss[7]) < float(loss[0])
    assert _same(dec.projection(), (W0, b0)) and dec._user_projection is None
    E1 = dec.class_table()[0]
    assert not torch.equal(E1, E0) and dec._source[2] is not None
    # projection only: the table is bit-identical, the projection moved
    dec.finetune(raw, labels, train_rows=False, **kw)
    assert _same(dec.class_table(), (E1, ids0))
    W1, b1 = dec.projection()
    assert not torch.equal(W1, W0) and not torch.equal(b1, b0)
    # both, and the stored head put back into a fresh decoder decodes bit for bit the same
    dec.finetune(raw, labels, **dict(kw, steps=150))
    W2, b2 = dec.projection()
    E2, ids2 = dec.class_table()
    assert not torch.equal(W2, W1) and not torch.equal(E2, E1)
    tuned = _probe(dec, raw)
    assert not torch.equal(tuned[2], model_out[2])
    twin = OnlineDecoder(engine, *norm, dtype=dtype)
    twin.set_projection(W2, b2)
    twin.set_classes(table=E2, ids=ids2)
    assert _same(_probe(twin, raw), tuned) and _same(twin.projection(), (W2, b2))
    # refresh keeps the user's head; reset_projection gives the model's back
    dec.refresh()
    assert _same(dec.projection(), (W2, b2)) and _same(_probe(dec, raw), tuned)
    dec.reset_projection()
    assert _same(dec.projection(), (W0, b0))
    dec.set_classes(IDS)
    assert _same(_probe(dec, raw), model_out)
    plain = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype)
    plain.refresh()                                              # without a user's projection refresh is what it was
    assert _same(_probe(plain, raw), model_out)
    # the installed head is the trained one: the loss of the logits a push returns has fallen on the recording it was given
    from contrastiveprosthetics_amd.finetune import class_weights
    from contrastiveprosthetics_amd.online import window_labels
    wl = window_labels(labels, 0)
    on = wl >= 0

    def loss_of(out):
        l = 4.0 * out[2].double().cpu().numpy()[on]
        nll = np.log(np.exp(l - l.max(1, keepdims=True)).sum(1)) + l.max(1) - l[np.arange(l.shape[0]), wl[on]]
        return float((class_weights(wl[on], 41) * nll).sum()), float((out[0].cpu().numpy()[on] == wl[on]).mean())

    (l0, acc0), (l1, acc1) = loss_of(model_out), loss_of(tuned)
    print(f"{dtype}: on the cued recording's own {int(on.sum())} labelled windows, balanced loss {l0:.4f} -> {l1:.4f}, "
          f"accuracy {acc0:.3f} -> {acc1:.3f} after 8 + 8 + 150 steps")
    assert l1 < l0


# ---------------------------------------------------------------------------------------------------------------- 5
def test_adaptive_form_keeps_its_statistics(engine, cued, norm):
    from contrastiveprosthetics_amd import OnlineDecoder
    raw, labels = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, adapt=0.05)
    dec.push(raw[:3000])                                         # the statistics have moved off the running ones
    stats = dec.bn_statistics()
    W0, b0 = dec.projection()
    assert float(b0.abs().max()) == 0.0                          # the unfolded projection has no bias
    E0 = dec.class_table()[0]
    counts, loss = dec.finetune(raw, labels, steps=6, lr=2e-3, lr_rows=2e-2, scale=4.0, min_windows=5, return_loss=True)
    assert torch.equal(dec.bn_statistics(), stats)               # fine-tuning never moves statistics
    assert bool(torch.isfinite(loss).all()) and float(loss[5]) < float(loss[0])
    W1, b1 = dec.projection()
    assert not torch.equal(W1, W0) and float(b1.abs().max()) > 0 and not torch.equal(dec.class_table()[0], E0)
    dec.refresh()
    assert _same(dec.projection(), (W1, b1)) and torch.equal(dec.bn_statistics(), stats)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("adaptive", [False, True])
def test_multi_stream_rows_match_the_single_stream_decoder(engine, cued, norm, adaptive):
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, MultiStreamDecoder, OnlineDecoder
    raw, labels = cued
    S, s_ft, alpha = 3, 1, 0.0
    kw = dict(steps=5, lr_rows=2e-2, scale=4.0, min_windows=5)

    def build():
        m = AdaptiveMultiStreamDecoder(engine, *norm, S, alpha) if adaptive else MultiStreamDecoder(engine, *norm, S)
        for s in range(S):
            m.set_classes(s, IDS)
        return m

    multi, twin = build(), build()                               # twin is never fine-tuned
    single = OnlineDecoder(engine, *norm, classes=IDS, adapt=alpha if adaptive else None)
    with pytest.raises(ValueError, match="shared by all streams"):
        multi.finetune(s_ft, raw, labels, train_projection=True, **kw)
    cm = multi.finetune(s_ft, raw, labels, **kw)
    cs = single.finetune(raw, labels, train_projection=False, **kw)
    assert cm == cs
    assert _same(multi.class_table(s_ft), single.class_table())
    assert not torch.equal(multi.class_table(s_ft)[0], twin.class_table(s_ft)[0])
    chunks = [raw[1000 * s:1000 * s + 1500] for s in range(S)]
    out, ref = multi.push(chunks, return_logits=True), twin.push(chunks, return_logits=True)
    for s in range(S):
        if s == s_ft:
            assert _same(out[s], single.push(chunks[s], return_logits=True)) and not torch.equal(out[s][2], ref[s][2])
        else:
            assert _same(multi.class_table(s), twin.class_table(s)) and _same(out[s], ref[s]), s


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("dtype,adapt", [("f32", None), ("bf16", None), ("f32", 0.05)])
def test_tail_inputs_do_not_depend_on_the_cut(engine, cued, norm, dtype, adapt):
    from contrastiveprosthetics_amd import OnlineDecoder
    from contrastiveprosthetics_amd.online import recording_windows
    raw, _ = cued
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, adapt=adapt)
    w = recording_windows(raw, dec.mean_std, dec._b, dec._a, 0).contiguous()
    n = int(w.shape[0])
    assert n > 400
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16

    def rows(cut, d=dec, key=None):
        u = torch.full((n, 512), float("nan"), dtype=tdt, device="cuda")
        for s in range(0, n, cut):
            m = min(cut, n - s)
            d._tail_inputs_call(key, w[s:].data_ptr(), m, u[s:].data_ptr(), *_scratch(d, m))
        torch.cuda.synchronize()
        return u

    whole = rows(n)
    assert bool(torch.isfinite(whole.float()).all()) and float(whole.float().abs().max()) > 0
    for cut in (1, 16, 333):
        assert torch.equal(rows(cut).view(torch.uint8), whole.view(torch.uint8)), cut
    # the multi-stream entry of the same form (cp_online_multi_tail_inputs / cp_online_multi_adapt_tail_inputs, a stream
    # that is not the first): the same rows as the single-stream decoder's, under the same cuts
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, MultiStreamDecoder
    multi = MultiStreamDecoder(engine, *norm, 3, dtype=dtype) if adapt is None \
        else AdaptiveMultiStreamDecoder(engine, *norm, 3, adapt, dtype=dtype)
    for cut in (n, 1, 16, 333):
        assert torch.equal(rows(cut, multi, 2).view(torch.uint8), whole.view(torch.uint8)), ("multi", cut)
