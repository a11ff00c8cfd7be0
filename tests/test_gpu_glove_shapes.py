"""The fused bf16 glove-angle class encoder (csrc/glove.cuh: glove_stats_kernel, glove_fwd_kernel, glove_bwd_kernel<0> and <1>) at
ragged row counts, against a plain torch float64 recomputation at the kernels' own rounding points.

Rows are R = 41 * groups, the forward kernels work in 16-row tiles and the backward kernels in 32-row pairs, so every group count
that is no multiple of 32 ends in a partial tile, and the kernels' tails rest on "rows past the end contribute zeros".  The shapes:

    groups      rows   what the tail looks like
         1        41   last tile 9 rows; the second pair has 9 rows and an EMPTY second tile
         2        82   last tile 2 rows
         3       123   last pair 27 rows
         7       287   last pair 31 rows (one short)
        25     1,025   last tile and last pair hold ONE row; the last forward workgroup has three idle waves
        32     1,312   41 pairs exactly (the aligned control)
      3201   131,241   just past all three grid caps (2,048 statistics tiles, 2,048 x 4 forward tiles, 512 backward pairs): every
                       stride loop takes more than one trip and the last trip is the ragged one; an odd group count >= 2,048 puts
                       the head in its two-groups-per-wave grid

The reference (`glove_reference`, `glove_backward_reference`): x, W1, W2 rounded to bf16; h = x W1^T; biased batch statistics over
the R rows (running statistics in stock-BN eval); scale = gamma / sqrt(var + eps), shift = beta - mean * scale; a = relu(scale h +
shift) rounded to bf16; zg = a W2^T.  Backward from the head's dL/dzg (torch autograd of the symmetric loss on the device's own z
and zg in f32, rounded to bf16 as the head stores it): g = [scale h + shift > 0] (dzg W2); dW2 = dzg^T a; dbeta = sum g; dgamma =
sum g hn; dh = BatchNorm backward, rounded to bf16; dW1 = dh^T x.  Loss and predictions: torch on the device's own z and zg (the
glove head).

Bars (max-error over max-reference): zg, dW1, dW2 <= 1e-3; dgamma, dbeta <= 1e-4; loss rel 2e-6; predictions >= 0.9999 agreement.
Where they come from: a torch f32 emulation of the kernels' arithmetic on the CPU (same rounding points, f32 sums and statistics)
deviated from this float64 reference by at most zg 2.9e-4, dW1 1.4e-4, dW2 5.3e-5, dgamma / dbeta 3e-7 at R = 41 .. 8,200 -- rare
one-ulp flips of the bf16-rounded a and dh where the f32 / f64 difference crosses a rounding boundary; 1e-3 is three times the
largest, ten times below the bars of the bench-size test against an un-rounded reference; 1e-4 leaves room for the `s2 - mean * s1`
cancellation in the kernel's f32 partial sums, which that emulation does not model.

Measured on the device (MI355X; max-error over max-reference, worst of stock BN / AdaBN):

        groups      rows        zg       dW1       dW2    dgamma     dbeta  loss rel
             1        41   1.1e-07   1.5e-05   1.9e-07   1.6e-07   1.2e-07   6.3e-08
             2        82   1.3e-07   3.3e-05   6.6e-08   1.1e-07   1.0e-07         0
             3       123   1.2e-07   1.5e-05   6.6e-08   1.2e-07   7.3e-08   6.4e-08
             7       287   4.7e-07   1.1e-04   1.2e-06   5.8e-07   4.5e-07   1.3e-07
            25     1,025   3.7e-05   1.4e-04   1.1e-05   2.8e-07   2.8e-07   6.4e-08
            32     1,312   1.7e-07   9.4e-05   1.8e-06   7.2e-07   6.4e-07   6.4e-08
          3201   131,241   4.8e-04   8.5e-06   6.5e-06   4.4e-06   4.6e-06         0
                     bar      1e-3      1e-3      1e-3      1e-4      1e-4      2e-6

predictions agree with torch's argmax at every shape (agreement 1.00000); the running mean / variance update holds at rtol 1e-4.
Eval at 3 groups x 25 samples: zg 1.3e-07 (stock BN) / 9.1e-08 (AdaBN), logits 2.2e-07 absolute, loss 4.0e-08 relative.
No bar was raised; the largest figure, zg 4.8e-04 at 131,241 rows, is one bf16 ulp of an `a` near the f32 / f64 rounding boundary
(the emulation's 2.9e-4 at 8,200 rows, over sixteen times as many elements).

The sensitivity guard runs on the reference alone: at every shape of at most 25 groups, taking the last valid row out of the
reference moves dW1, dW2 and that row of zg by more than three times their bar -- a kernel that dropped (or doubled) the tail row
could not pass.  At 131,241 rows one row is below the bar for the weight gradients: that shape pins the stride loops and every
forward row, the small shapes pin the tail.
"""
import numpy as np
import pytest
import torch

from test_gpu_glove import glove_state, make_engine, step
from test_gpu_parity import T

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1                       # the engine's cp_config.bn_eps / bn_momentum
W1_KEY, W2_KEY = "glove_net.linear.1.weight", "glove_net.last.0.weight"
BAR = {"zg": 1e-3, "dW1": 1e-3, "dW2": 1e-3, "dgamma": 1e-4, "dbeta": 1e-4}
SHAPES = (1, 2, 3, 7, 25, 32, 3201)


def bn_base(adabn):
    return "glove_net.linear.2" + (".bn" if adabn else "")


def state(seed, adabn):
    """glove_state (non-trivial BN affine) with non-trivial running statistics for the class encoder's stock BatchNorm"""
    sd = glove_state(seed, adabn)
    if not adabn:
        g = torch.Generator().manual_seed(seed + 3)
        sd[bn_base(False) + ".running_mean"] = 0.3 * torch.randn(256, generator=g)
        sd[bn_base(False) + ".running_var"] = 0.5 + torch.rand(256, generator=g)
    return sd


def data(B, seed, V=1):
    """class-structured windows and glove rows (a class mean plus noise), as the bench-size test draws them"""
    g = torch.Generator().manual_seed(seed)
    mu_e, mu_g = torch.randn(T, 12, generator=g), torch.randn(T, 20, generator=g)
    EMG = (mu_e[None, :, None] + torch.randn(B, T, V, 12, generator=g)).reshape(B, T, V, 1, 12)
    GLOVE = mu_g[None] + 0.3 * torch.randn(B, T, 20, generator=g)
    return EMG, GLOVE, torch.arange(T).repeat(B)


def bf(t):
    """round to bf16 (nearest even, from f32 as the kernels do), back in float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def rel(got, ref):
    return float((got.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


def glove_reference(e, adabn, GLOVE, running=None):
    """float64 forward of the class encoder at the kernels' rounding points, on the GPU; running = (mean, var) for stock-BN eval"""
    V = e.values.views
    r = {"x": bf(GLOVE.reshape(-1, 20).cuda()), "W2": bf(V[W2_KEY])}
    h = r["x"] @ bf(V[W1_KEY]).t()
    if running is None:
        r["mean"], r["var"] = h.mean(0), h.var(0, unbiased=False)
    else:
        r["mean"], r["var"] = running[0].double(), running[1].double()
    r["invstd"] = 1.0 / torch.sqrt(r["var"] + EPS)
    r["scale"] = V[bn_base(adabn) + ".weight"].double() * r["invstd"]
    bn = r["scale"] * h + (V[bn_base(adabn) + ".bias"].double() - r["mean"] * r["scale"])
    r["h"], r["mask"], r["a"] = h, bn > 0, bf(torch.relu(bn))
    del bn
    r["zg"] = r["a"] @ r["W2"].t()
    return r


def glove_backward_reference(r, dzg):
    """the four gradients from dL/dzg (R,16), plus the last row's own terms of the two weight gradients (the sensitivity guard)"""
    R = r["h"].shape[0]
    dzg = bf(dzg)
    g = r["mask"] * (dzg @ r["W2"])
    hn = (r["h"] - r["mean"]) * r["invstd"]
    out = {"dW2": dzg.t() @ r["a"], "dbeta": g.sum(0), "dgamma": (g * hn).sum(0)}
    dh = bf(r["scale"] * (g - out["dbeta"] / R - hn * (out["dgamma"] / R)))
    del g, hn
    out["dW1"] = dh.t() @ r["x"]
    out["last_row"] = {"dW1": dh[-1][:, None] * r["x"][-1][None, :], "dW2": dzg[-1][:, None] * r["a"][-1][None, :]}
    return out


def head_reference(z, zg, B, V, want_grad):
    """the symmetric loss, predictions and logits by torch on the device's own z (window order b, t, v) and zg; f32 with autograd for
    dL/dzg (training, V = 1), float64 without"""
    dt = torch.float32 if want_grad else torch.float64
    zt = z.detach().to(dt).clone().requires_grad_(want_grad)
    zgt = zg.detach().to(dt).clone().requires_grad_(want_grad)
    zn = (zt / zt.norm(dim=-1, keepdim=True)).reshape(B, T, V, 16).permute(0, 2, 1, 3)         # (B, V, T, 16)
    cn = (zgt / zgt.norm(dim=-1, keepdim=True)).reshape(B, 1, T, 16)
    logits = (zn @ cn.transpose(2, 3)).reshape(B * V, T, T)
    tgt = torch.arange(T, device=z.device).repeat(B * V)
    loss = (torch.nn.functional.cross_entropy(logits.reshape(-1, T), tgt)
            + torch.nn.functional.cross_entropy(logits.transpose(1, 2).reshape(-1, T), tgt)) / 2
    if want_grad:
        loss.backward()
    return loss.item(), logits.detach(), (zgt.grad if want_grad else None)


@pytest.mark.parametrize("adabn", [False, True])
@pytest.mark.parametrize("B", SHAPES)
def test_fused_glove_training_step_vs_fp64_recompute(B, adabn):
    """one bf16 training step per shape of the module's table: zg, the four class-encoder gradients, loss and predictions against
    the reference; stock BN also the running mean / variance update (the f32 test's tolerance, rtol 1e-4)"""
    R = B * T
    e = make_engine(state(61 + int(adabn), adabn), adabn, "bf16")
    EMG, GLOVE, label = data(B, 800 + B + 100 * int(adabn))
    gb = bn_base(adabn)
    before = None if adabn else {k: e.running_state()[gb + k].clone() for k in (".running_mean", ".running_var")}
    x = EMG.reshape(-1, 12).cuda()
    e.grads.flat.zero_()
    z = e.encoder_forward(x, training=True)
    zg = e.glove_forward(GLOVE.cuda(), training=True)
    out, pred, _ = e.head_glove(z, zg, label.cuda(), 1, want_grad=True)
    e.encoder_backward(x)
    e.glove_backward()
    torch.cuda.synchronize()
    assert tuple(zg.shape) == (R, 16) and torch.isfinite(zg).all() and torch.isfinite(e.grads.flat).all()

    r = glove_reference(e, adabn, GLOVE)
    loss_ref, logits_ref, dzg = head_reference(z, zg, B, 1, True)
    ref = glove_backward_reference(r, dzg)
    ref["zg"] = r["zg"]
    G = e.grads.views
    got = {"zg": zg, "dW1": G[W1_KEY], "dW2": G[W2_KEY], "dgamma": G[gb + ".weight"], "dbeta": G[gb + ".bias"]}
    err = {k: rel(got[k], ref[k]) for k in BAR}
    agree = float((pred.reshape(-1).long() == logits_ref.argmax(-1).reshape(-1)).float().mean())
    loss_rel = abs(out[0].item() - loss_ref) / abs(loss_ref)
    print(f"\nfused glove step, {B} groups ({R} rows), {'AdaBN' if adabn else 'stock BN'}: "
          + ", ".join(f"{k} {v:.1e}" for k, v in err.items()) + f", loss rel {loss_rel:.1e}, pred agreement {agree:.5f}")

    if B <= 25:                                 # the sensitivity guard: the reference without its last valid row
        moved = {k: float(ref["last_row"][k].abs().max()) / float(ref[k].abs().max()) for k in ("dW1", "dW2")}
        moved["zg"] = float(ref["zg"][-1].abs().max()) / float(ref["zg"].abs().max())
        print("  the last row alone moves: " + ", ".join(f"{k} {v:.1e}" for k, v in moved.items()))
        for k, v in moved.items():
            assert v > 3 * BAR[k], ("a dropped tail row would pass unseen", k, v)

    for k in BAR:
        assert err[k] <= BAR[k], (k, err[k])
    assert out[0].item() == pytest.approx(loss_ref, rel=2e-6)
    assert agree >= 0.9999, agree
    if not adabn:
        rs = e.running_state()
        unbiased = r["var"] * (R / (R - 1))
        for k, stat in ((".running_mean", r["mean"]), (".running_var", unbiased)):
            want = (1 - MOMENTUM) * before[k].double() + MOMENTUM * stat
            np.testing.assert_allclose(rs[gb + k].cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-6)


def test_fused_glove_eval_rows_do_not_depend_on_the_batch_cut():
    """bf16, stock BN, eval (running statistics): a row's zg depends on its own 20 inputs and the folded statistics alone, so the rows
    of a batch of 1, 7 or 25 groups are bit-identical to the same rows inside the 32-group batch -- from its start, and from group 5
    on (row 205 = 12 tiles + 13: every row changes its place inside a tile, its wave and its workgroup)"""
    e = make_engine(state(62, False), False, "bf16")
    _, GLOVE, _ = data(32, 900)
    GLOVE = GLOVE.cuda()
    whole = e.glove_forward(GLOVE, training=False).clone()
    assert torch.isfinite(whole).all() and float(whole.abs().max()) > 0
    for B in (1, 7, 25):
        for first in (0, 5):
            part = e.glove_forward(GLOVE[first:first + B], training=False)
            torch.cuda.synchronize()
            assert tuple(part.shape) == (B * T, 16)
            assert torch.equal(part, whole[first * T:(first + B) * T]), (B, first)


@pytest.mark.parametrize("adabn", [False, True])
def test_fused_glove_eval_adabn_and_vote_expansion(adabn):
    """bf16 eval at 3 groups x 25 samples: 3,075 windows against 123 class rows.  Stock BN folds the running statistics; AdaBN takes
    the batch-statistics path with no padded copy of x written.  zg against the reference (the bf16 bar); logits, predictions and
    loss against torch on the device's own z and zg at the bars of the f32 eval test"""
    B, V = 3, 25
    e = make_engine(state(63, adabn), adabn, "bf16")
    EMG, GLOVE, label = data(B, 1000, V)
    gb = bn_base(adabn)
    running = None if adabn else tuple(e.running_state()[gb + k].clone() for k in (".running_mean", ".running_var"))
    z = e.encoder_forward(EMG.reshape(-1, 12).cuda(), training=False)              # (step() without the backward, keeping z)
    zg = e.glove_forward(GLOVE.cuda(), training=False)
    out, pred, logits = e.head_glove(z, zg, label.cuda(), V, want_grad=False, want_logits=True)
    torch.cuda.synchronize()
    r = glove_reference(e, adabn, GLOVE, running)
    err = rel(zg, r["zg"])
    loss_ref, logits_ref, _ = head_reference(z, zg, B, V, False)
    print(f"\nfused glove eval, {B} groups x {V} samples, {'AdaBN' if adabn else 'stock BN'}: zg {err:.1e}, "
          f"logits {float((logits.double() - logits_ref).abs().max()):.1e}, loss rel {abs(out[0].item() - loss_ref) / abs(loss_ref):.1e}")
    assert tuple(zg.shape) == (B * T, 16) and tuple(logits.shape) == (B * V, T, T)
    assert err <= BAR["zg"], err
    np.testing.assert_allclose(logits.cpu().numpy(), logits_ref.cpu().numpy(), atol=3e-5, rtol=0)
    assert np.array_equal(pred.cpu().numpy(), logits_ref.argmax(-1).cpu().numpy())
    assert out[0].item() == pytest.approx(loss_ref, rel=3e-6)
    if not adabn:                                # eval leaves the running statistics alone
        for k, v in zip((".running_mean", ".running_var"), running):
            assert torch.equal(e.running_state()[gb + k], v), k


def test_stale_workspace_rows_are_never_read():
    """a bf16 step at 64 groups, then one at 7 groups on the same engine: the workspaces keep the larger batch's rows past R = 287
    (x copy, dL/dzg, partial sums, weight-gradient slabs).  The 7-group step must be bit-identical to the same step on a fresh
    engine: the `row < R` guards hold, and the slab and partial sums run in a fixed order (reproducible)"""
    sd = state(64, False)
    EMG_a, GLOVE_a, label_a = data(64, 1100)
    EMG_b, GLOVE_b, label_b = data(7, 1101)
    keys = (W1_KEY, bn_base(False) + ".weight", bn_base(False) + ".bias", W2_KEY)

    def run(e):
        x = EMG_b.reshape(-1, 12).cuda()
        e.grads.flat.zero_()
        z = e.encoder_forward(x, training=True)
        zg = e.glove_forward(GLOVE_b.cuda(), training=True)
        out, pred, _ = e.head_glove(z, zg, label_b.cuda(), 1, want_grad=True)
        e.encoder_backward(x)
        e.glove_backward()
        torch.cuda.synchronize()
        return z.clone(), zg.clone(), out.clone(), {k: e.grads.views[k].clone() for k in keys}

    used = make_engine(sd, False, "bf16")
    step(used, EMG_a, GLOVE_a, label_a)
    z1, zg1, out1, g1 = run(used)
    z0, zg0, out0, g0 = run(make_engine(sd, False, "bf16"))
    assert torch.isfinite(zg0).all() and all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in g0.values())
    assert torch.equal(z1, z0)                   # first: a difference in the sEMG encoder is not the glove kernels'
    assert torch.equal(zg1, zg0)
    assert torch.equal(out1[0], out0[0])
    for k in keys:
        assert torch.equal(g1[k], g0[k]), k
