"""The learnable temperature of the contrastive head (cp_head_temp / cp_head_glove_temp: head_kernel<..., TEMP = true>,
head_finalize_kernel's column 658, reduce_rows_kernel in front of it), the head called on its own with the input recipe, seeds,
poisoned workspaces and NaN-filled gradient store of tests/test_gpu_head.py, against the float64 reference of
tests/head_temperature_ref.py (anchored by tests/test_head_temperature_host.py); then through Model, GraphStep and two shards.

    s = logit_scale, S = ln 100, tau = exp(clamp(s, -S, S)); logits = tau * cosines; dz_hat, dE_hat carry tau;
    dL/ds = sum dl * logits inside [-S, S], 0 outside.

Group counts, the smallest at which each launch shape occurs: 1, 5 (the smallest launches), 257 (65 blocks: reduce_rows_kernel must
carry column 658), 2049 (two groups per wave with a ragged tail: the new accumulator is reused across groups), 6 with V = 3
(gradients at V > 1), 75 with V = 25 (evaluation, no gradients).  Forms: one-hot f32 / bf16, glove f32 / bf16, 8-bit logits at 5 and
2049; labels arange and the permutation that is no involution.

(a) off is off: cp_head_temp at s = 0 against cp_head on the same inputs, every output bit for bit (glove twin likewise).
(b) against float64 at s in {ln 0.5, ln 1/0.07, ln 100, 5.0}; "ln 100" is the largest float32 inside [-S, S] (float32(ln 100) lies
    above ln 100), 5.0 is clamped: every output bit of the ln 100 run, dL/ds exactly 0.  Bars, m = max(1, tau):
        logits              2e-5 * m absolute (8-bit logits: 2e-4 * m against the e4m3 emulation times tau)
        loss                2e-6 relative;   loss_correct[1] exact
        predictions         exact on every row whose float64 COSINE top-2 margin exceeds 4e-5 (the same rows for every tau); at most
                            0.2 % of a case's rows left out (the host module checks the cap on the CPU: <= 0.057 %, 0.195 % at 75 x 25)
        d_easy_w, d_easy_b  2e-4 of the tensor's largest entry
        dL/dz, dL/dzg       every row against its own largest reference entry: 4 x the worst row of a plain torch float32 evaluation
                            of the same formulas on these inputs (temp_reference(dtype=torch.float32) on the CPU, every f32 case),
                            plus 2^-8 of the entry in 16-bit storage
        dL/ds               |error| / sum |dl * logits| of the reference: 4 x the same float32 torch baseline
    The float32 torch baselines, measured on the CPU per tau (worst f32 case of each kind, 1 .. 2049 groups and 6 x 3):
        tau                           0.5        1/0.07     100 (and the clamped run)
        dz / dzg row (BASE_DZ)        8.4e-07    3.1e-06    9.6e-01
        dz / dzg group (BASE_DZN)     6.3e-07    7.4e-07    2.8e-06
        dL/ds (BASE_DS)               1.6e-08    9.3e-08    6.4e-08
        logits / m                    1.5e-07    3.2e-07    3.3e-07       (bar 2e-5)
        loss rel                      7.7e-08    1.3e-07    1.9e-07       (bar 2e-6)
        d_easy_w, d_easy_b            9.9e-07    2.4e-06    1.3e-06       (bar 2e-4)
    No baseline exceeds half of a project bar (logits, loss, table gradients) at any tau, so those stay as stated.
    At tau = 100 the row-by-row rule says little: a row whose softmax has saturated has a gradient below the float32 resolution of
    p - 1, and the float32 torch evaluation itself misses such rows by 96 % of their largest entry (glove, 2049 groups), so four
    times that baseline admits anything.  The rule is kept as stated and a second check is added beside it, with a baseline that
    is small at every tau: rows times the length of the input row they differentiate (dL/dz_i * |z_i|: the gradient with respect
    to the direction, free of the 10^[-3, 3] row scales) against the largest such entry of their batch entry, 4 x BASE_DZN, plus
    2^-8 of the entry in 16-bit storage.
    Sensitivity, on the reference alone: dL/ds summed without the last group misses its bar; dz without the factor tau misses the
    row bar at tau = 1/0.07.
(c) through Model (f32, no dropout, 8 groups): three training steps of Model(temperature=1/0.07) against a subclass of
    oracle.ref_cpu.OracleModel whose forward multiplies the logits by exp(s) and whose class-side Adam holds s -- first loss 2e-6
    relative, the three losses 5e-4, s after step k within 2e-3 * lr_glove * k (tests/test_gpu_parity.py's bars); the state_dict
    round trip keeps s; an evaluation's loss uses tau; a model built without the argument has logit_scale.grad None, no table
    entry, and the loss bits of cp_head called directly.
(d) GraphStep with a learnt temperature equals the eager step bit for bit over three replays, and s moves.
(e) two shards: the mean of the two half-batches' dL/ds equals the full batch's (each shard's loss is a mean over ITS groups, as
    under data parallelism, where the step averages the summed gradients) within the table-gradient bar.
(f) a NULL logit_scale and global negatives with a temperature are refused.

Measured on the device (MI355X), worst over the cases of a kind and over the four scales unless a scale is named (every case prints
its own lines); the 2 s of the whole module are mostly the float64 references:

    kind           logits / m  loss rel  dz row (0.5 | 1/0.07)  dz group (0.5 | 1/0.07 | 100)   dzg group  table grads  dL/ds (0.5 | 1/0.07 | 100)
    one-hot f32    5.9e-07     4.9e-07   1.0e-06 | 6.6e-06      7.6e-07 | 7.9e-07 | 3.1e-06        -        1.5e-06      2.9e-08 | 8.4e-08 | 2.3e-07
    glove f32      5.6e-07     5.5e-07   1.0e-06 | 5.4e-06 dzg  8.3e-07 | 9.8e-07 | 2.8e-06     3.0e-06        -         1.4e-08 | 5.3e-08 | 1.7e-07
    one-hot bf16   as f32      as f32    3.89e-03               3.86e-03                           -        as f32       1.5e-08 | 4.9e-08 | 1.1e-07
    glove bf16     as f32      as f32    3.89e-03               3.83e-03                        3.86e-03       -         as f32
    8-bit logits   6.5e-05     8.6e-08   3.88e-03               3.85e-03                           -        1.2e-06      1.4e-08 | 3.4e-08 | 5.9e-08
    bar            2e-5 (2e-4) 2e-6      3.4e-06 | 1.2e-05      2.5e-06 | 3.0e-06 | 1.1e-05     (same)      2e-4         6.4e-08 | 3.7e-07 | 2.6e-07
                                         (+ 2^-8 of the entry in 16-bit storage: 3.91e-03)
    dz row at tau = 100: 1.06 of the row's largest entry (bar 3.8, see above); rows left out <= 0.045 %, 0.195 % at 75 x 25.
(a): no word differed in any case.  The clamped run equalled the run at the bound in every word, with dL/ds = 0.  (c): losses 7.1449389 /
7.0174270 / 6.3760624 against the oracle's 7.1449394 / 7.0175376 / 6.3774338; s 2.6566072, 2.6539593, 2.6513379 on both sides.
(d): s 2.65926 -> 2.65661 -> 2.65414 -> 2.65183, eager and graph alike.  (e): shards 6.3937950 and 6.7658896, mean 6.5798423, full batch
6.5798426, float64 6.5798427.
"""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_temperature_ref as tr  # noqa: E402  (tests/head_temperature_ref.py)
from test_gpu_head import Case, W_KEY, B_KEY  # noqa: E402  (the input recipe and seeds of tests/test_gpu_head.py)
from oracle import head_cpu as hc  # noqa: E402
from oracle import ref_cpu as oc  # noqa: E402

pytestmark = pytest.mark.gpu

T = 41
LOGITS_BAR, FP8_LOGITS_BAR, LOSS_BAR, TABLE_GRAD_BAR = 2e-5, 2e-4, 2e-6, 2e-4
MARGIN, EXCLUDED_CAP = 4e-5, 0.002
BF16_STEP = 2.0 ** -8
# float32 torch baselines per scale (CPU, worst f32 case; module docstring); "5.0" is the clamped run: the figures of "ln 100"
BASE_DZ = {"ln 0.5": 8.4e-7, "ln 1/0.07": 3.1e-6, "ln 100": 9.6e-1}
BASE_DZN = {"ln 0.5": 6.3e-7, "ln 1/0.07": 7.4e-7, "ln 100": 2.8e-6}
BASE_DS = {"ln 0.5": 1.6e-8, "ln 1/0.07": 9.3e-8, "ln 100": 6.4e-8}
BASE_DZ["5.0"], BASE_DZN["5.0"], BASE_DS["5.0"] = BASE_DZ["ln 100"], BASE_DZN["ln 100"], BASE_DS["ln 100"]
CP_ERR_ARG = 10001
BEST = dict(d_e=16, lr_emg=9.761e-4, reg_emg=7.103e-5, dp_emg=0.0, lr_glove=2.653e-3, reg_glove=2.840e-6, dp_glove=0.0)

CASES = ([Case("onehot", "f32", G) for G in (1, 5, 257, 2049)] +
         [Case("onehot", "f32", G, layout="perm") for G in (5, 257)] +
         [Case("onehot", "bf16", G) for G in (5, 257, 2049)] +
         [Case("glove", "f32", G) for G in (1, 5, 257, 2049)] +
         [Case("glove", "f32", 5, layout="perm")] +
         [Case("glove", "bf16", G) for G in (5, 257, 2049)] +
         [Case("fp8", "fp8", G) for G in (5, 2049)] +
         [Case("onehot", dt, 6, V=3, layout="perm") for dt in ("f32", "bf16")] +
         [Case("onehot", "f32", 75, V=25, layout="perm", want_grad=False)])
IDS = [c.id for c in CASES]

_engines = {}


def engine(dtype, class_encoder, temp):
    from contrastiveprosthetics_amd.engine import Engine
    key = (dtype, class_encoder, temp)
    if key not in _engines:
        _engines[key] = Engine(adabn=True, dtype=dtype, device="cuda", class_encoder=class_encoder, temperature=1.0 if temp else None)
    return _engines[key]


def run_head(case, inp, s=None):
    """the head on its own: poisoned workspaces and gradient store, one call, everything it left behind; s=None: the engine
    without a temperature (cp_head / cp_head_glove)"""
    from contrastiveprosthetics_amd import _lib
    glove = case.variant == "glove"
    e = engine(case.dtype, "glove" if glove else "onehot", s is not None)
    z, labels = inp["z"].cuda(), inp["labels"].cuda()
    n = z.shape[0]
    e.values.views[W_KEY].copy_(inp["w"])
    e.values.views[B_KEY].copy_(inp["b"])
    e.grads.flat.fill_(float("nan"))
    if s is not None:
        e.logit_scale.fill_(s)
        assert float(e.logit_scale) == s                               # (a float32 value, taken exactly)
    e.workspace(n)[(_lib.FP8_STATE_BYTES if case.dtype == "fp8" else 0):].fill_(0xFF)
    if glove:
        zg = inp["zg"].cuda()
        e._gws_args(zg.shape[0])
        e._gws.fill_(0xFF)
        out, pred, logits = e.head_glove(z, zg, labels, case.V, want_grad=case.want_grad, want_logits=True)
    else:
        out, pred, logits = e.head(z, labels, case.V, want_grad=case.want_grad, want_logits=True)
    got = dict(loss=out[0].clone(), correct=out[1].clone(), pred=pred, logits=logits)
    if case.want_grad:
        got["dz"] = e.debug_head_grad()
        if glove:
            got["dzg"] = e.debug_glove_head_grad()
        else:
            got["d_easy_w"], got["d_easy_b"] = e.grads.views[W_KEY].clone(), e.grads.views[B_KEY].clone()
        if s is not None:
            got["ds"] = e.d_logit_scale.clone()
    torch.cuda.synchronize()
    return got


def bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_off_is_off(case):
    """(a) cp_head_temp / cp_head_glove_temp at s = 0 leave the bits of cp_head / cp_head_glove"""
    inp = case.inputs()
    plain, temp = run_head(case, inp), run_head(case, inp, 0.0)
    keys = [k for k in plain]
    assert set(temp) - set(plain) <= {"ds"}
    differ = {k: int((bits(plain[k]) != bits(temp[k])).sum()) for k in keys if not same_bits(plain[k], temp[k])}
    print(f"\noff-is-off {case.id:26s} compared {keys}: differing elements {differ}")
    assert not differ
    assert not torch.isnan(plain["logits"]).any() and (not case.want_grad or not torch.isnan(plain["dz"]).any())
    if case.want_grad:
        assert torch.isfinite(temp["ds"])


def rows_within(got, ref, dtype, base):
    """(every row within its bar, worst row error over that row's largest reference entry); NaN fails"""
    got, rowmax = got.double(), ref.abs().max(dim=1, keepdim=True).values
    err = (got - ref).abs()
    allowed = 4 * base * rowmax + (0.0 if dtype == "f32" else BF16_STEP) * ref.abs()
    return bool((err <= allowed).all()), float((err / rowmax).max())


def groups_within(got, ref, inputs, B, dtype, base):
    """rows times |input row| against the largest such entry of their batch entry -> (all within the bar, worst figure)"""
    n = inputs.double().norm(dim=1, keepdim=True)
    g, r = (got.double() * n).reshape(B, -1), (ref * n).reshape(B, -1)
    err, top = (g - r).abs(), r.abs().max(dim=1, keepdim=True).values
    allowed = 4 * base * top + (0.0 if dtype == "f32" else BF16_STEP) * r.abs()
    return bool((err <= allowed).all()), float((err / top).max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_head_temperature_against_float64(case):
    """(b)"""
    inp = case.inputs()
    dev = {k: v.cuda() for k, v in inp.items()}
    G, V, y = case.groups, case.V, dev["labels"][:T]
    cls = dict(zg=dev["zg"]) if case.variant == "glove" else dict(easy_w=dev["w"], easy_b=dev["b"])
    runs, lines, fails = {}, [], []
    for name, s in tr.SCALES.items():
        got = runs[name] = run_head(case, inp, s)
        tau = tr.tau_of(s)
        m = max(1.0, tau)
        true = tr.temp_reference(dev["z"], dev["labels"], V, s, want_grad=case.want_grad, **cls)
        fig = {}

        def bar(key, value, limit):
            fig[key] = value
            if not value <= limit:              # (NaN fails)
                fails.append(f"[{name}] {key} {value:.3e} > {limit:.1e}")

        if case.variant == "fp8":
            zh = dev["z"] / dev["z"].norm(dim=-1, keepdim=True)
            E = dev["w"].t() + dev["b"][None]
            q = lambda t: t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32)
            emu = (q(zh).reshape(G, T, 16) @ q(E / E.norm(dim=-1, keepdim=True)).t()[None]).double() * tau
            bar("logits/m", float((got["logits"].double() - emu).abs().max()) / m, FP8_LOGITS_BAR)
            ref = tr.temp_from_logits(got["logits"], dev["z"], dev["labels"], V, s, dev["w"], dev["b"])
            margin = ref["logits"].topk(2, dim=-1).values
            margin = (margin[..., 0] - margin[..., 1]) / tau
        else:
            bar("logits/m", float((got["logits"].double() - true["logits"]).abs().max()) / m, LOGITS_BAR)
            ref, margin = true, true["margin"]
        bar("loss rel", abs(float(got["loss"]) - float(ref["loss"])) / float(ref["loss"]), LOSS_BAR)
        keep = margin > MARGIN
        bar("excluded rows", 1.0 - float(keep.double().mean()), EXCLUDED_CAP)
        bar("wrong predictions", float((got["pred"][keep].long() != ref["pred"][keep]).sum()), 0)
        bar("correct count off by", abs(float(got["correct"]) - float((got["pred"] == y[None]).sum())), 0)
        if case.want_grad:
            for k in ("dz", "dzg") if case.variant == "glove" else ("dz",):
                assert got[k].shape == (ref[k].shape[0], 64)
                bar(k + " cols 16..63 non-zero", float((got[k][:, 16:] != 0).sum()), 0)
                ok, worst = rows_within(got[k][:, :16], ref[k], case.dtype, BASE_DZ[name])
                fig[k + " row"] = worst
                if not ok:
                    fails.append(f"[{name}] {k}: worst row error {worst:.3e} of the row's largest entry (f32 bar {4 * BASE_DZ[name]:.1e})")
                ok, worst = groups_within(got[k][:, :16], ref[k], dev["z" if k == "dz" else "zg"], G // V, case.dtype, BASE_DZN[name])
                fig[k + " group"] = worst
                if not ok:
                    fails.append(f"[{name}] {k}: worst entry {worst:.3e} of its batch entry's largest, rows times |input row| "
                                 f"(f32 bar {4 * BASE_DZN[name]:.1e})")
                if name == "ln 1/0.07":
                    assert not rows_within(ref[k] / tau, ref[k], case.dtype, BASE_DZ[name])[0], f"{k} without the factor tau would pass"
                    assert not groups_within(ref[k] / tau, ref[k], dev["z" if k == "dz" else "zg"], G // V, case.dtype, BASE_DZN[name])[0]
            if case.variant != "glove":
                for k in ("d_easy_w", "d_easy_b"):
                    bar(k, float((got[k].double() - ref[k]).abs().max()) / float(ref[k].abs().max()), TABLE_GRAD_BAR)
            scale = float(ref["abs_dl_l"])
            bar("ds", abs(float(got["ds"]) - float(ref["ds"])) / scale, 4 * BASE_DS[name])
            if name != "5.0":
                assert abs(float(ref["dl_l"][:-1].sum()) - float(ref["ds"])) / scale > 4 * BASE_DS[name], \
                    "dL/ds summed without the last group would pass"
            else:
                bar("ds of the clamped run", abs(float(got["ds"])), 0)
        lines.append(f"head-temp {case.id:24s} s {name:9s} | " + "  ".join(
            f"{k} {100 * v:.3f} %" if k == "excluded rows" else f"{k} {v:.2e}" for k, v in fig.items()
            if v != 0 or k in ("logits/m", "loss rel", "excluded rows", "ds")))
    print("\n" + "\n".join(lines))
    # the clamped run: every output bit of the run at the bound
    a, b = runs["ln 100"], runs["5.0"]
    differ = [k for k in a if k != "ds" and not same_bits(a[k], b[k])]
    if differ:
        fails.append(f"s = 5.0 differs from s = ln 100 in {differ}")
    assert not fails, "; ".join(fails)


# ---- (c) through the model ------------------------------------------------------------------------------------------------
class TempOracle(oc.OracleModel):
    """OracleModel with the temperature: logits = exp(clamp(s)) * cosines, s = sd["logit_scale"] in the class-side Adam"""

    def forward(self, EMG, GLOVE, labels, *a, **k):
        cos = super().forward(EMG, GLOVE, labels, *a, **k)
        return torch.exp(torch.clamp(self.sd["logit_scale"], -tr.S_MAX, tr.S_MAX)) * cos

    def make_optimizers(self):
        emg, glove = oc.trainable_keys(self.sd)
        opt_e = torch.optim.Adam([self.sd[k] for k in emg], lr=self.params["lr_emg"], weight_decay=0)
        opt_g = torch.optim.Adam([self.sd[k] for k in glove] + [self.sd["logit_scale"]], lr=self.params["lr_glove"], weight_decay=0)
        return opt_e, opt_g


def randn(seed, shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_model_trains_the_temperature():
    from contrastiveprosthetics_amd.models import Model
    tau0, B = 1 / 0.07, 8
    model = Model(BEST, adabn=True, dtype="f32", seed=17, temperature=tau0)
    e = model.engine
    assert list(e.specs)[-1] == "logit_scale" and list(model.state_dict())[0] == "logit_scale"
    assert model.logit_scale.data_ptr() == e.values.views["logit_scale"].data_ptr() and model.logit_scale.requires_grad
    assert float(model.logit_scale) == pytest.approx(math.log(tau0), rel=1e-7) and model.temperature() == pytest.approx(tau0, rel=1e-6)
    sd = oc.init_state_dict(17, 16, True)                            # the oracle's own initialisation on both sides, s = ln tau0
    sd["logit_scale"] = model.logit_scale.detach().cpu().clone()
    model.load_state_dict(sd)
    ref = TempOracle(sd, BEST, adabn=True, requires_grad=True)
    opts = ref.make_optimizers()
    label = torch.arange(T).repeat(B)
    model.set_train()
    got_losses, ref_losses, s_moves = [], [], []
    for k in range(3):
        EMG = randn(300 + k, (B, T, 1, 1, 12))
        ref_losses.append(ref.train_step(EMG, torch.zeros(B, T, 20), label, opts))
        logits = model.forward(EMG.cuda(), None, label.cuda())
        loss = model.loss(logits, label.cuda())
        model.backward()
        model.optimizer_step()
        got_losses.append(float(loss))
        s_got, s_ref = float(model.logit_scale), float(ref.sd["logit_scale"])
        s_moves.append((s_got, s_ref))
        print(f"step {k}: loss {got_losses[-1]:.7f} (oracle {ref_losses[-1]:.7f})  s {s_got:.7f} (oracle {s_ref:.7f}, "
              f"off by {abs(s_got - s_ref) / (BEST['lr_glove'] * (k + 1)):.2e} of lr * step)")
    assert got_losses[0] == pytest.approx(ref_losses[0], rel=2e-6)
    assert got_losses == pytest.approx(ref_losses, rel=5e-4)
    for k, (s_got, s_ref) in enumerate(s_moves):
        assert abs(s_got - s_ref) <= 2e-3 * BEST["lr_glove"] * (k + 1), (k, s_got, s_ref)
    assert s_moves[-1][0] != s_moves[0][0] != math.log(tau0)
    # through autograd: named["logit_scale"].grad is filled like every other entry
    logits = model.forward(randn(310, (B, T, 1, 1, 12)).cuda(), None, label.cuda())
    model.zero_grad()
    model.loss(logits, label.cuda()).sum().backward()
    named = dict(model.named_parameters())
    assert named["logit_scale"].grad is not None and float(named["logit_scale"].grad) == float(e.d_logit_scale) != 0.0
    # state_dict round trip keeps s
    state = {k: v.clone() for k, v in model.state_dict().items()}
    twin = Model(BEST, adabn=True, dtype="f32", seed=1, temperature=3.0)
    twin.load_state_dict(state)
    assert float(twin.logit_scale) == float(model.logit_scale) == float(twin.engine.logit_scale)
    fixed = Model(BEST, adabn=True, dtype="f32", seed=1, temperature=3.0, learn_temperature=False)
    assert "logit_scale" not in fixed.engine.specs and not fixed.logit_scale.requires_grad
    fixed.load_state_dict(state)
    assert float(fixed.engine.logit_scale) == float(model.logit_scale) and list(fixed.state_dict())[0] == "logit_scale"
    # an evaluation's loss uses tau: the logits are tau times those of a model without the option on the same weights
    plain = Model(BEST, adabn=True, dtype="f32", seed=1)
    plain.load_state_dict(state)                                      # (its logit_scale is loaded and, as ever, not used)
    EMG = randn(320, (2, T, 3, 1, 12)).cuda()
    lab = torch.arange(T).repeat(2).cuda()
    tau = model.temperature()
    out = {}
    for name, mdl in (("plain", plain), ("twin", twin)):
        mdl.set_test()
        with torch.no_grad():
            lg = mdl.forward(EMG, None, lab)
            out[name] = (lg.clone(), float(mdl.loss(lg, lab)))
    assert float((out["twin"][0].double() - tau * out["plain"][0].double()).abs().max()) <= LOGITS_BAR * max(1.0, tau)
    want = float(hc.loss_of_logits(out["twin"][0].double(), lab))
    assert out["twin"][1] == pytest.approx(want, rel=LOSS_BAR) and abs(out["twin"][1] - out["plain"][1]) > 0.1


def test_model_without_the_option_is_the_model_of_before():
    from contrastiveprosthetics_amd.engine import Engine
    from contrastiveprosthetics_amd.models import Model
    B = 8
    model = Model(BEST, adabn=True, dtype="f32", seed=17)
    e = model.engine
    assert e.logit_scale is None and "logit_scale" not in e.specs and model.temperature() is None
    EMG, label = randn(300, (B, T, 1, 1, 12)).cuda(), torch.arange(T).repeat(B).cuda()
    model.set_train()
    logits = model.forward(EMG, None, label)
    loss = model.loss(logits, label)
    loss.sum().backward()
    named = dict(model.named_parameters())
    assert named["logit_scale"].grad is None and float(model.logit_scale) == 0.0 and list(model.state_dict())[0] == "logit_scale"
    # the same weights through cp_head itself, called here
    e2 = Engine(adabn=True, dtype="f32", device="cuda")
    e2.load_named(model.state_dict())
    x = EMG.reshape(-1, 12)
    z = e2.encoder_forward(x, training=True)
    cfg = e2._cfg(x.shape[0], True)
    ws, nb = e2._ws_args(cfg)
    out = torch.empty(2, device="cuda")
    pred = torch.empty(B, T, dtype=torch.int32, device="cuda")
    lg = torch.empty(B, T, T, device="cuda")
    rc = e2.lib.cp_head(C.byref(cfg), C.byref(e2._p), z.data_ptr(), label.data_ptr(), B, 1, 1, ws, nb, out.data_ptr(), pred.data_ptr(),
                        lg.data_ptr(), C.byref(e2._g), e2._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert same_bits(out[0:1], loss.detach().reshape(1)) and same_bits(lg, logits)
    assert torch.equal(e2.grads.views[W_KEY], e.grads.views[W_KEY])


# ---- (d) graph step ---------------------------------------------------------------------------------------------------------
def test_graph_step_with_a_learnt_temperature():
    from contrastiveprosthetics_amd.engine import Engine, GraphStep
    from test_gpu_graph_step import data
    table, emg_rand, perms = data()
    labels = torch.arange(T).repeat(8).cuda()
    res = []
    for mode in ("eager", "graph"):
        e = Engine(adabn=True, dtype="f32", dp_emg=0.0, device="cuda", seed=3, temperature=1 / 0.07)
        e.init_parameters(11)
        losses, ss = [], [float(e.logit_scale)]
        if mode == "graph":
            gs = GraphStep(e, table, emg_rand, 8, BEST)
            assert float(e.logit_scale) == ss[0]                     # (the warm-up step was rolled back)
        for perm in perms[:3]:
            if mode == "graph":
                losses.append(gs.step(perm)[0].item())
            else:
                x = e.gather(table, emg_rand, perm, 1)
                z = e.encoder_forward(x, training=True)
                out, _, _ = e.head(z, labels, 1, want_grad=True)
                e.encoder_backward(x)
                e.adam_step(BEST)
                losses.append(out[0].item())
            ss.append(float(e.logit_scale))
        torch.cuda.synchronize()
        res.append((e, losses, ss))
    (a, la, sa), (b, lb, sb) = res
    print(f"\nlosses {la} | s {sa}")
    assert la == lb and sa == sb
    assert torch.equal(a.values.flat, b.values.flat) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert len(set(sb)) == 4                                         # s moved in every replay: the graph reads it from the device


# ---- (e) two shards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_shards_sum_to_the_full_batch(dtype):
    case = Case("onehot", dtype, 10)
    inp = case.inputs()
    s = tr.SCALES["ln 1/0.07"]
    full = run_head(case, inp, s)
    half = Case("onehot", dtype, 5)
    parts = []
    for r in range(2):
        sl = slice(r * 5 * T, (r + 1) * 5 * T)
        shard = dict(inp, z=inp["z"][sl].contiguous(), labels=inp["labels"][sl].contiguous(), zg=inp["zg"][sl].contiguous())
        parts.append(run_head(half, shard, s))
    dev = {k: v.cuda() for k, v in inp.items()}
    ref = tr.temp_reference(dev["z"], dev["labels"], 1, s, easy_w=dev["w"], easy_b=dev["b"])
    mean = (float(parts[0]["ds"]) + float(parts[1]["ds"])) / 2        # (the step's grad_scale = 1 / world)
    print(f"\nshards {float(parts[0]['ds']):.7e} + {float(parts[1]['ds']):.7e} -> {mean:.7e}; full {float(full['ds']):.7e}; float64 {float(ref['ds']):.7e}")
    scale = max(abs(float(ref["ds"])), 1e-30)
    assert abs(mean - float(full["ds"])) <= TABLE_GRAD_BAR * scale and abs(mean - float(ref["ds"])) <= TABLE_GRAD_BAR * scale
    assert abs(float(parts[0]["ds"]) - float(full["ds"])) > TABLE_GRAD_BAR * scale      # (one shard alone is not the batch)
    w = (parts[0]["d_easy_w"] + parts[1]["d_easy_w"]).double() / 2
    assert float((w - ref["d_easy_w"]).abs().max()) <= TABLE_GRAD_BAR * float(ref["d_easy_w"].abs().max())


# ---- (f) refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from contrastiveprosthetics_amd.models import Model
    case = Case("onehot", "f32", 5)
    inp = case.inputs()
    e = engine("f32", "onehot", True)
    z, labels = inp["z"].cuda(), inp["labels"].cuda()
    cfg = e._cfg(z.shape[0], False)
    ws, nb = e._ws_args(cfg)
    out, pred = torch.empty(2, device="cuda"), torch.empty(5, T, dtype=torch.int32, device="cuda")
    d = torch.zeros((), device="cuda")
    args = (C.byref(cfg), C.byref(e._p), z.data_ptr(), labels.data_ptr(), 5, 1)
    tail = (ws, nb, out.data_ptr(), pred.data_ptr(), None, C.byref(e._g))
    assert e.lib.cp_head_temp(*args, 1, *tail, None, d.data_ptr(), e._stream()) == CP_ERR_ARG
    assert b"logit_scale" in e.lib.cp_last_error()
    assert e.lib.cp_head_temp(*args, 1, *tail, e.logit_scale.data_ptr(), None, e._stream()) == CP_ERR_ARG
    assert e.lib.cp_head_temp(*args, 0, *tail, e.logit_scale.data_ptr(), None, e._stream()) == 0       # (no gradients: not needed)
    eg = engine("f32", "glove", True)
    zg = inp["zg"].cuda()
    gws, gnb = eg._gws_args(zg.shape[0])
    cfg = eg._cfg(z.shape[0], False)
    ws, nb = eg._ws_args(cfg)
    assert eg.lib.cp_head_glove_temp(C.byref(cfg), z.data_ptr(), zg.data_ptr(), labels.data_ptr(), 5, 1, 1, ws, nb, gws, gnb,
                                     out.data_ptr(), pred.data_ptr(), None, None, d.data_ptr(), eg._stream()) == CP_ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="tau"):
        Model(BEST, adabn=True, dtype="f32", global_negatives=True, temperature=2.0)
    with pytest.raises(NotImplementedError, match="tau"):
        e.global_negatives(z, labels)
    with pytest.raises(NotImplementedError, match="tau"):
        e.head(z, labels, 1, want_grad=False, gneg=torch.zeros(2, 64, device="cuda"))
