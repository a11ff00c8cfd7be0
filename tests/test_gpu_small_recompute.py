"""The small-batch kernels (csrc/small.cuh: sm_prep_kernel, sm_fc_fwd_kernel, sm_fc_bwd_kernel, sm_reduce_grads_kernel; the `small`
branches of the conv kernels and of conv_backward_tail) launch by launch, at the ragged sizes where the path changes shape, against
a torch float64 recomputation of EACH launch's output from THAT launch's own stored inputs, rounded where the kernel rounds.

One training step (forward, head with want_grad, backward) runs with cp_config.grad_tap set from before the forward; the forward
record must say the small path ran.  Inputs are read back through debug_activation, debug_bn_stats, the tap (include/cpnative.h:
slot L = 2..8 the masked dL/d(BN_L output), slot 9 the same for conv2's BatchNorm as fc1's launch wrote it, slot 1 what conv2's
weight-gradient launch wrote over it, slot 0 the stand-alone data-gradient launch, slot 10 dz as the head stored it), z and the
parameters.  "round" = round-to-nearest-even to bf16 (f32: the identity):

  forward   conv1: r0 = round(relu(b + w . x));  conv2: round(relu(conv(round(r0 s + t) zero-padded, round(W2)) + b2))
            fc:    u = round(mask / (1-p) (r s + t)), s, t = the stored scale / shift, mask read as test_dropout_replay_f32 reads it;
                   out = round(relu(u round(W)^T + b));  projection z = u round(W)^T in f32
            stored mean / invstd of every layer against the float64 mean / biased variance of the stored activation, scale / shift
            against gamma, beta and those; stock BN: the running update (momentum 0.1, unbiased variance)
  backward  fc launch L: Gin = slot L, r_L, the statistics of L; s1 = sum Gin, s2 = sum Gin r_L (float64);
                   A' = round([r_L > 0] (ca Gin + cb r_L + cz));  dgamma = (s2 - mean s1) invstd, dbeta = s1, db = sum A',
                   dW = A'^T u_{L-1} (fc1: column k = c 12 + w),  Gout = round(mask / (1-p) (A' round(W))) against the next slot.
                   Above 24 groups (128-feature tiles, no k split) the bf16 tile is rounded once more on its way through LDS:
                   Gout = round(mask / (1-p) round(A' round(W))), which the reference does too.
            projection: the same with A' = slot 10
            conv tail: BatchNorm2's gamma / beta from slot 9; slot 1 = round([r2 > 0] (ca g + cb r2 + cz)); conv2's bias gradient
                   (sums of slot 1) and weight gradient (kernel rows 0 and 2 exactly zero); slot 0 = round(conv2's data gradient of
                   slot 1 with round(W2)); BatchNorm1's gamma / beta and conv1's gradients from the unrounded data gradient
  ReLU masks are the device's own (r > 0 of the stored activation): no comparison depends on the side of zero of a pre-activation.

Shapes (rows N = 41 groups).  The host arithmetic they follow (csrc/encoder_api.cuh, encoder_forward_small_t / encoder_backward_small_t;
mirrored by host_plan() below, which the test asserts against this table):
    row tiles   tiles_m = ceil(N / 32) (SM_BM);  k split (64-feature tiles, wave pairs) while tiles_m * 8 <= 256, i.e. N <= 1,024
    row splits  s0 = min(8, ceil(N / 256));  rows per split rps = ceil(ceil(N / s0) / 64) * 64;  splits = ceil(N / rps)

    groups   rows  tiles_m  last tile  k split  splits  rps  last split   why
         1     41        2          9      yes       1   64          41   second row tile holds 9 rows; BatchNorm over 41 rows
         6    246        8         22      yes       1  256         246   largest whole-batch weight gradient
         7    287        9         31      yes       2  192          95   first 2-split case; the second split ends inside a 64-row step
        24    984       31         24      yes       4  256         216   last size on k-split tiles
        25  1,025       33          1       no       5  256           1   first size on 128-feature tiles; last tile and last split hold ONE row
        64  2,624       82         32       no       7  384         320   dispatch limit
Cases: bf16 stock BN at every size with dp in {0, 0.0635}; bf16 AdaBN at 7 and 25 groups; f32 at 1 and 25 groups; evaluation under
AdaBN (which takes the small forward too) at 2 x 25 groups in bf16, forward checks only.

Bars.  The reference rounds where the kernel rounds, so what is left is the f32 accumulation order (against float64) and one-step
disagreements where the two land on different sides of a rounding boundary.  The model:
    stored bf16 tensors   every element within 2^-7 |ref| + 1e-3 rms(ref): one bf16 step (2^-6, two steps, for the twice-rounded Gout
                          under dropout above 24 groups); rms error <= 1e-3 rms(ref); the share of bit-identical elements is printed
    stored f32 tensors    max error <= 1e-5 max |ref|
    f32 sums of exact products (weight / bias gradients, z): 5e-5 of the tensor's maximum; gamma / beta gradients 1e-5;
    mean rtol 2e-4 (atol 2e-5), invstd rtol 2e-3 (the bars of tests/test_gpu_fullsize.py, recompute_check)
    unstored roundings    the operands u and A' are rounded to bf16 INSIDE a launch and never stored, so the device's copy cannot
                          be read.  Where the float64 value of such an element lies within f32 distance of a bf16 rounding boundary
                          the device's element is one step above or below the reference's, and everything the launch computes
                          from it moves by that step times the other factor (a weight gradient: one step of A' times a row of u,
                          2e-5 .. 4.5e-4 of its maximum, against 1.2e-7 in a launch without such an element).  amb() marks those
                          elements -- distance to a boundary within 2^-22 relative for the fma chains, for A' also within the
                          distance between the launch's own totals, which it writes out as dgamma / dbeta, and the float64 sums --
                          and exactly the outputs such an element reaches get `step x |other factor|` added to their bar
                          (a worked example: amb's docstring).  Elements no ambiguous rounding reaches, the majority, are held to
                          the plain bar and reported separately.
Asserted: BAR, each value with model -> measured -> asserted (about ten times the measured worst, never above the model).

Guards on the reference alone (7 and 25 groups): with the last valid row's A' (forward: operand) zeroed, dW, db and that row of
Gout / the activation move by at least 10 x the bound enforced on the same elements, allowance included -- a dropped tail row
cannot pass.

Measured on the MI355X, per case: the first ten figures of the `summary` line _print() prints (the worst figure of each kind
over the case's launches).  fwd act / Gout: worst element in units of its bound (f32: max error over max |ref|) and the smallest
share of bit-identical elements; rms: largest rms error over rms(ref); z, dW, db, gamma / beta: max error over max |ref| where no
ambiguous rounding reaches; last: the largest dW error where one does (inside its allowance).  The printed line ends with the largest
error / (bar + allowance) and the smallest guard ratio of the case, which depend on the asserted bars: at 7 and 25 groups every guard
ratio printed was at least 62 (a row of Gout at 25 groups with dropout).

    bf16, stock BN, dp 0.0, 1 groups = 41 rows, training step               | fwd act 0.5 | fwd act identical 0.99995 | Gout 0.76 | Gout identical 0.99986 | rms 2.6e-05 | z 2.4e-07 | dW 1.3e-07 | db 2.1e-07 | gamma/beta 6.6e-08 | dW where a rounding is ambiguous 3.2e-07
    bf16, stock BN, dp 0.0635, 1 groups = 41 rows, training step            | fwd act 0.36 | fwd act identical 0.99986 | Gout 0.51 | Gout identical 0.99967 | rms 1.2e-05 | z 1.4e-07 | dW 1.5e-07 | db 3.2e-07 | gamma/beta 1.2e-07 | dW where a rounding is ambiguous 2.2e-05
    bf16, stock BN, dp 0.0, 6 groups = 246 rows, training step              | fwd act 0.77 | fwd act identical 0.99993 | Gout 0.78 | Gout identical 0.99960 | rms 5.3e-05 | z 1.3e-07 | dW 1.8e-07 | db 2.1e-07 | gamma/beta 9e-08 | dW where a rounding is ambiguous 8.6e-05
    bf16, stock BN, dp 0.0635, 6 groups = 246 rows, training step           | fwd act 0.78 | fwd act identical 0.99948 | Gout 0.8 | Gout identical 0.99918 | rms 0.0001 | z 1.4e-07 | dW 2.2e-07 | db 3.7e-07 | gamma/beta 1.1e-07 | dW where a rounding is ambiguous 0.00045
    bf16, stock BN, dp 0.0, 7 groups = 287 rows, training step              | fwd act 0.92 | fwd act identical 0.99993 | Gout 0.87 | Gout identical 0.99967 | rms 7e-05 | z 1.9e-07 | dW 1.5e-07 | db 1.8e-07 | gamma/beta 1.7e-07 | dW where a rounding is ambiguous 7.1e-05
    bf16, stock BN, dp 0.0635, 7 groups = 287 rows, training step           | fwd act 0.92 | fwd act identical 0.99980 | Gout 0.65 | Gout identical 0.99990 | rms 9.9e-05 | z 2.5e-07 | dW 1.7e-07 | db 3e-07 | gamma/beta 1.3e-07 | dW where a rounding is ambiguous 0.00031
    bf16, stock BN, dp 0.0, 24 groups = 984 rows, training step             | fwd act 0.88 | fwd act identical 0.99995 | Gout 0.84 | Gout identical 0.99965 | rms 3.6e-05 | z 2.7e-07 | dW 2e-07 | db 2.3e-07 | gamma/beta 9.9e-08 | dW where a rounding is ambiguous 0.00012
    bf16, stock BN, dp 0.0635, 24 groups = 984 rows, training step          | fwd act 0.93 | fwd act identical 0.99985 | Gout 0.91 | Gout identical 0.99989 | rms 4.9e-05 | z 1.9e-07 | dW 2.7e-07 | db 2.3e-07 | gamma/beta 1.1e-07 | dW where a rounding is ambiguous 6.8e-05
    bf16, stock BN, dp 0.0, 25 groups = 1025 rows, training step            | fwd act 0.89 | fwd act identical 0.99993 | Gout 0.8 | Gout identical 0.99983 | rms 2.7e-05 | z 2.5e-07 | dW 1.4e-07 | db 2.7e-07 | gamma/beta 1.4e-07 | dW where a rounding is ambiguous 7.6e-05
    bf16, stock BN, dp 0.0635, 25 groups = 1025 rows, training step         | fwd act 0.89 | fwd act identical 0.99992 | Gout 0.9 | Gout identical 0.99986 | rms 3.2e-05 | z 1.7e-07 | dW 1.9e-07 | db 1.2e-07 | gamma/beta 7.4e-08 | dW where a rounding is ambiguous 3.9e-05
    bf16, stock BN, dp 0.0, 64 groups = 2624 rows, training step            | fwd act 0.94 | fwd act identical 0.99995 | Gout 0.94 | Gout identical 0.99988 | rms 3.5e-05 | z 2e-07 | dW 2.1e-07 | db 2.7e-07 | gamma/beta 9.4e-08 | dW where a rounding is ambiguous 0.0001
    bf16, stock BN, dp 0.0635, 64 groups = 2624 rows, training step         | fwd act 0.94 | fwd act identical 0.99979 | Gout 0.92 | Gout identical 0.99987 | rms 5.7e-05 | z 2e-07 | dW 1.7e-07 | db 3.3e-07 | gamma/beta 1e-07 | dW where a rounding is ambiguous 0.00019
    bf16, AdaBN, dp 0.0635, 7 groups = 287 rows, training step              | fwd act 0.92 | fwd act identical 0.99980 | Gout 0.65 | Gout identical 0.99990 | rms 9.9e-05 | z 2.5e-07 | dW 1.7e-07 | db 3e-07 | gamma/beta 1.3e-07 | dW where a rounding is ambiguous 0.00031
    bf16, AdaBN, dp 0.0635, 25 groups = 1025 rows, training step            | fwd act 0.89 | fwd act identical 0.99992 | Gout 0.9 | Gout identical 0.99986 | rms 3.2e-05 | z 1.7e-07 | dW 1.9e-07 | db 1.2e-07 | gamma/beta 7.4e-08 | dW where a rounding is ambiguous 3.9e-05
    f32, stock BN, dp 0.0635, 1 groups = 41 rows, training step             | fwd act 4.9e-07 | fwd act identical - | Gout 3.9e-07 | Gout identical - | rms - | z 5.6e-07 | dW 4.1e-07 | db 3.3e-07 | gamma/beta 3.1e-07 | dW where a rounding is ambiguous -
    f32, stock BN, dp 0.0635, 25 groups = 1025 rows, training step          | fwd act 1.1e-06 | fwd act identical - | Gout 6.6e-07 | Gout identical - | rms - | z 7.5e-07 | dW 4e-07 | db 5.5e-07 | gamma/beta 2.6e-07 | dW where a rounding is ambiguous -
    bf16, AdaBN, dp 0.0635, 50 groups = 2050 rows, evaluation, forward only | fwd act 0.88 | fwd act identical 0.99994 | Gout - | Gout identical - | rms 3.3e-05 | z 1.9e-07 | dW - | db - | gamma/beta - | dW where a rounding is ambiguous -

Scratch builds whose bounds only drop work (never committed, never out of range): DESIGN.md 7e-2, last paragraph.
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_fullsize import LIN, _bn_names, _shift_w

pytestmark = pytest.mark.gpu

T = 41
EPS, MOMENTUM = 1e-5, 0.1                       # the engine's cp_config.bn_eps / bn_momentum
P_DROP = 0.0635

# asserted bars: model value -> measured worst over the 17 cases -> asserted (about 10 x the measured worst, never above the model)
BAR = {
    "step": 2.0 ** -7,          # one bf16 step, relative: structural, not a measurement (measured worst element: 0.94 of its bar)
    "abs": 1e-3,                # ... plus this share of rms(ref) (model; part of the same element bar)
    "rms": 1e-3,                # rms error of a stored bf16 tensor over rms(ref): model 1e-3, measured <= 1.0e-4
    "f32": 1e-5,                # stored f32 tensor, max error over max |ref|: model 1e-5, measured <= 1.1e-6
    "wgrad": 5e-6,              # weight gradients, z: model 5e-5, measured <= 2.7e-7 (bf16), 7.5e-7 (f32)
    "bgrad": 5e-6,              # bias gradients: model 5e-5, measured <= 3.7e-7 (bf16), 5.5e-7 (f32)
    "bn": 3e-6,                 # gamma / beta gradients: model 1e-5, measured <= 1.7e-7 (bf16), 3.1e-7 (f32)
    "mean_rtol": 2e-6, "mean_atol": 2e-7,       # model 2e-4 / 2e-5, measured 6.5e-4 of that
    "invstd_rtol": 3e-6,                        # model 2e-3, measured 2.4e-7
    "running_rtol": 5e-6, "running_atol": 5e-8,       # the f32 update of the running statistics: started at 1e-4 / 1e-6, measured 4.5e-3 of that
    "head_f32": 5e-6,           # the f32 head's stored dz against float64 autograd (a check of the INPUT): started at 2e-4, measured 4.3e-7
}

#        groups: (rows, tiles_m, last tile, k split, splits, rows per split, last split)
TABLE = {1: (41, 2, 9, True, 1, 64, 41), 6: (246, 8, 22, True, 1, 256, 246), 7: (287, 9, 31, True, 2, 192, 95),
         24: (984, 31, 24, True, 4, 256, 216), 25: (1025, 33, 1, False, 5, 256, 1), 64: (2624, 82, 32, False, 7, 384, 320)}


def host_plan(N):
    """tile and split counts as encoder_forward_small_t / encoder_backward_small_t derive them (SM_BM = 32, sm_ksplit)"""
    tiles_m = (N + 31) // 32
    s0 = min(8, (N + 255) // 256)
    rps = ((N + s0 - 1) // s0 + 63) // 64 * 64
    splits = (N + rps - 1) // rps
    return (N, tiles_m, N - 32 * (tiles_m - 1), tiles_m * 8 <= 256, splits, rps, N - rps * (splits - 1))


SUMMARY = "summary"                             # key of the per-case worst figures inside a report


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def small_recompute_check(groups, dtype, adabn, dp, train=True):
    """one step at `groups` groups, every launch against its float64 recomputation; prints the table of measured errors (also when
    a bar fails: every figure is recorded before it is asserted)"""
    report = {}
    try:
        _recompute(report, groups, dtype, adabn, dp, train)
    finally:
        _print(report, groups, T * groups, dtype, adabn, dp, train)
    return report


def _recompute(report, groups, dtype, adabn, dp, train):
    from contrastiveprosthetics_amd.engine import Engine
    B, N = groups, T * groups
    bf16 = dtype == "bf16"
    drop = train and dp > 0
    if groups in TABLE:
        assert host_plan(N) == TABLE[groups], (host_plan(N), TABLE[groups])
    ksplit = host_plan(N)[3]
    guard = train and groups in (7, 25)

    def rnd(t):
        return t.to(torch.float32).to(torch.bfloat16).to(torch.float64) if bf16 else t.to(torch.float64)

    e = Engine(adabn=adabn, dtype=dtype, dp_emg=dp, device="cuda", seed=1000)
    e.init_parameters(5)
    gen = torch.Generator().manual_seed(9)
    bnn = _bn_names(adabn)
    W, G = e.values.views, e.grads.views
    for b in bnn:                                                   # non-trivial affine, as recompute_check sets it
        W[b + ".weight"].copy_((1.0 + 0.2 * torch.randn(W[b + ".weight"].shape, generator=gen)).cuda())
        W[b + ".bias"].copy_((0.1 * torch.randn(W[b + ".bias"].shape, generator=gen)).cuda())
    before = {}
    if not adabn:                                                   # ... and non-trivial running statistics
        for b in bnn:
            e.running[b + ".running_mean"].copy_((0.3 * torch.randn(e.running[b + ".running_mean"].shape, generator=gen)).cuda())
            e.running[b + ".running_var"].copy_((0.5 + torch.rand(e.running[b + ".running_var"].shape, generator=gen)).cuda())
            before[b] = (e.running[b + ".running_mean"].double().clone(), e.running[b + ".running_var"].double().clone())
    g_ = torch.Generator().manual_seed(6 + groups)
    mu_ = torch.randn(T, 12, generator=g_)
    if train:
        x = (mu_[None, :, :] + torch.randn(B, T, 12, generator=g_)).reshape(N, 12).cuda()
    else:                                                           # evaluation: V = 2 samples per (group, class), window order (b, t, v)
        x = (mu_[None, :, None, :] + torch.randn(B // 2, T, 2, 12, generator=g_)).reshape(N, 12).cuda()
    labels = torch.arange(T).repeat(B).cuda()
    tdt = torch.bfloat16 if bf16 else torch.float32
    tap = torch.full((11, N, 768), float("nan"), dtype=tdt, device="cuda")       # exactly the 11 slots the small path asks for
    e.grad_tap = tap
    e.grads.flat.zero_()
    z = e.encoder_forward(x, training=train)
    assert e._rec.path == 1 and e._rec.n_windows == N, ("the small path did not run", e._rec.path)     # PATH_SMALL
    if train:
        out, _, _ = e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
    torch.cuda.synchronize()
    e.grad_tap = None
    assert torch.isfinite(z).all() and torch.isfinite(e.grads.flat).all()

    steps_abs, rms_bar = BAR["abs"], BAR["rms"]
    summary = report.setdefault(SUMMARY, {})

    def worst(key, value, fn=max):
        """the case's summary line (_print): the worst figure of each kind over the case's launches"""
        summary[key] = fn(summary[key], value) if key in summary else value

    def amb(pre, delta):
        """where the device's rounding of an UNSTORED intermediate may differ from the reference's: the bf16 step of every element of
        `pre` (float64, before rounding) that lies within `delta` of a rounding boundary -- `delta` bounds how far the device's f32
        value can be from `pre` -- and zero elsewhere (f32: nothing is rounded).  Such an element is one step off or not; what it
        may move downstream is added to that tensor's bar, element by element, and to no other element's.
        Worked example: pre = 0.40137 lies in [2^-2, 2^-1), where bf16 values are ulp = 2^-9 = 0.001953 apart; pre / ulp = 205.5014,
        so pre is 0.0014 ulp = 2.7e-6 above the boundary between 205 ulp and 206 ulp.  An operand element has delta = 2^-22 |pre| =
        9.6e-8 < 2.7e-6: not ambiguous, amb = 0.  An A' element whose coefficients carry, say, delta = 4e-6 is ambiguous: amb = ulp,
        and a weight-gradient element dW[f][k] that this A'[m][f] reaches gets ulp * |u[m][k]| = 0.00195 * 0.8 = 1.6e-3 added to its
        bar -- against a dropped row's A'[m][f] * u[m][k] = 0.32, 200 times as much."""
        if not bf16:
            return torch.zeros_like(pre)
        a = pre.abs()
        ulp = torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 7)
        q = a / ulp
        dist = (q - torch.floor(q) - 0.5).abs() * ulp
        return torch.where((dist <= delta) & (a > 0), ulp, torch.zeros_like(ulp))

    def check_act(name, got, ref, steps=1, allow=None):
        """a stored tensor of the compute dtype.  bf16: worst element in units of its bar (steps * 2^-7 |ref| + 1e-3 rms(ref) [+ allow]),
        rms error over rms(ref), share of bit-identical elements; f32: max error over max |ref|"""
        got, ref = got.double(), ref.double()
        err = (got - ref).abs()
        rr = _rms(ref) + 1e-300
        if bf16:
            bound = steps * BAR["step"] * ref.abs() + steps_abs * rr
            raw = float((err / bound).max())
            wst = float((err / (bound + allow)).max()) if allow is not None else raw
            rms = _rms(err) / rr
            same = float((got == ref).double().mean())
            report[name] = "worst/bar %.2f  rms %.1e  identical %.5f" % (wst, rms, same) + ("" if allow is None else "  (without the allowance %.2f)" % raw)
            kind = "fwd act" if name.startswith("fwd/") else "Gout"
            worst(kind, wst), worst(kind + " identical", same, min), worst("rms", rms)
            assert wst <= 1.0 and rms <= rms_bar, (name, wst, rms, same)
        else:
            a = float(err.max()) / (float(ref.abs().max()) + 1e-300)
            report[name] = "max %.1e" % a
            worst("fwd act" if name.startswith("fwd/") else "Gout", a)
            assert a <= BAR["f32"], (name, a)

    def check_param(name, got, ref, bar, allow=None):
        """an f32 result: max error over max |ref| against BAR[bar]; with `allow`, every element against BAR[bar] max |ref| + allow"""
        err = (got.double() - ref.double()).abs()
        mx = float(ref.abs().max()) + 1e-300
        a = float(err.max()) / mx
        kind = "z" if name.endswith(" z") else "dW" if name.endswith(" dW") else "db" if name.endswith(" db") else "gamma/beta" if bar == "bn" else None
        if allow is None or float(allow.max()) == 0.0:
            report[name] = "max %.1e  (bar %.0e)" % (a, BAR[bar])
            if kind:
                worst(kind, a)
            assert a <= BAR[bar], (name, a, BAR[bar])
            return
        clean = allow == 0                                           # elements no ambiguous rounding can reach
        a0 = float(err[clean].max()) / mx if bool(clean.any()) else 0.0
        wst = float((err / (BAR[bar] * mx + allow)).max())
        report[name] = "max %.1e  (bar %.0e)  where no ambiguous rounding reaches; elsewhere %.1e, error/(bar + allowance) %.2f, %d elements" % (
            a0, BAR[bar], a, wst, int((~clean).sum()))
        if kind:
            worst(kind, a0), worst(kind + " where a rounding is ambiguous", a), worst("error/(bar + allowance)", wst)
        assert wst <= 1.0, (name, a, wst)

    def moved_enough(name, delta, ref_row, ref, steps=1, allow_row=None):
        """guard: some element of the last row moves by 10 x the bound check_act enforces on THAT element (its allowance
        included) when the row's input is taken out (reference only)"""
        if not guard:
            return
        if bf16:
            bound = steps * BAR["step"] * ref_row.abs() + steps_abs * _rms(ref) + (allow_row if allow_row is not None else 0.0)
            ratio = float((delta.abs() / bound).max())
        else:
            ratio = float(delta.abs().max()) / (BAR["f32"] * float(ref.abs().max()) + 1e-300)
        report[name + " | guard: last row moves (x its bound)"] = "%.0f" % ratio
        worst("guard", ratio, min)
        assert ratio >= 10.0, ("a dropped tail row would pass unseen", name, ratio)

    def moved_param(name, delta, ref, bar, allow=None):
        """the same for an f32 result: the last row's own term against BAR[bar] max |ref| + allow of the same elements"""
        if not guard:
            return
        bound = BAR[bar] * float(ref.abs().max()) + (allow if allow is not None else 0.0) + 1e-300
        ratio = float((delta.abs() / bound).max())
        report[name + " | guard: last row moves (x its bound)"] = "%.0f" % ratio
        worst("guard", ratio, min)
        assert ratio >= 10.0, ("a dropped tail row would pass unseen", name, ratio)

    F32_OPS = 2.0 ** -22          # bound on the relative distance of a short f32 fma chain from its float64 value (each step 2^-24)
    st = [e.debug_bn_stats(l).double() for l in range(9)]           # [mean, invstd, scale, shift] per BatchNorm
    thresh = min(65535.0, max(1.0, float(int(dp * 65536.0 + 0.5))))
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(thresh) / np.float32(65536.0))) if drop else 1.0

    def check_stats(l, act, count):
        """stored statistics of layer l against the float64 moments of the stored activation `act` (rows x channels)"""
        C = act.shape[1]
        mean, var = act.mean(0), act.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + EPS)
        gamma, beta = W[bnn[l] + ".weight"].double(), W[bnn[l] + ".bias"].double()
        em = float(((st[l][0] - mean).abs() / (BAR["mean_rtol"] * mean.abs() + BAR["mean_atol"])).max())
        ei = float(((st[l][1] - invstd).abs() / (BAR["invstd_rtol"] * invstd)).max())
        # scale = gamma * invstd and shift = beta - mean * scale in f32 from the STORED mean / invstd: a rounding each
        es = float(((st[l][2] - gamma * st[l][1]).abs() / (2.0 ** -23 * (gamma * st[l][1]).abs() + 1e-30)).max())
        et = float(((st[l][3] - (beta - st[l][0] * st[l][2])).abs() / (2.0 ** -22 * (beta.abs() + (st[l][0] * st[l][2]).abs()) + 1e-30)).max())
        report["fwd/stats%d (mean, invstd, scale, shift: error / bar)" % l] = "%.1e  %.1e  %.2f  %.2f" % (em, ei, es, et)
        assert em <= 1 and ei <= 1 and es <= 1 and et <= 1, (l, em, ei, es, et)
        assert act.shape[0] == count and C == st[l].shape[1]
        if train and not adabn:
            rm, rv = e.running[bnn[l] + ".running_mean"].double(), e.running[bnn[l] + ".running_var"].double()
            want_m = (1 - MOMENTUM) * before[bnn[l]][0] + MOMENTUM * mean
            want_v = (1 - MOMENTUM) * before[bnn[l]][1] + MOMENTUM * var * (count / (count - 1.0))
            er = max(float(((rm - want_m).abs() / (BAR["running_rtol"] * want_m.abs() + BAR["running_atol"])).max()),
                     float(((rv - want_v).abs() / (BAR["running_rtol"] * want_v.abs() + BAR["running_atol"])).max()))
            report["fwd/running%d (error / bar)" % l] = "%.1e" % er
            assert er <= 1, (l, er)

    # ---------------- forward: conv stage ------------------------------------------------------------------------------
    r0 = e.debug_activation(0).double().reshape(N, 12, 64)           # conv1's output as its consumers recompute it
    w1 = W["emg_net.conv_emg.0.weight"][:, 0, 1, :].double()          # (64, 3): only kernel row 1 meets data
    xp = torch.nn.functional.pad(x.double(), (1, 1))
    taps = torch.stack([xp[:, t:t + 12] for t in range(3)], -1)       # (N, 12, 3)
    check_act("fwd/conv1", r0, rnd(torch.relu(taps @ w1.t() + W["emg_net.conv_emg.0.bias"].double())))
    check_stats(0, r0.reshape(-1, 64), N * 12)
    u1x = r0 * st[0][2] + st[0][3]                                   # BatchNorm1's output, exact; the image holds it rounded
    u1, u1a = rnd(u1x), amb(u1x, F32_OPS * u1x.abs())
    wc2 = W["emg_net.conv_emg.3.weight"][:, :, 1, :].double()        # (co, ci, tap)
    wc2r = rnd(wc2)
    r1 = e.debug_activation(1).double().reshape(N, 12, 64)
    pre = sum(_shift_w(u1, t - 1) @ wc2r[:, :, t].t() for t in range(3)) + W["emg_net.conv_emg.3.bias"].double()
    check_act("fwd/conv2", r1, rnd(torch.relu(pre)), allow=sum(_shift_w(u1a, t - 1) @ wc2r[:, :, t].abs().t() for t in range(3)))
    check_stats(1, r1.reshape(-1, 64), N * 12)
    del pre

    # ---------------- forward: fc1..fc7 and the projection ---------------------------------------------------------------
    acts = {1: r1.reshape(N, 768)}
    for L in range(2, 9):
        acts[L] = e.debug_activation(L).double()
    keep = {}
    for Lp in range(1, 9):
        keep[Lp] = None
        if drop and Lp >= 5:
            bn = acts[Lp] * st[Lp][2] + st[Lp][3]
            keep[Lp] = ((e.debug_activation(9 + Lp - 5) != 0) | (bn == 0)).double()
            kr, p = float(keep[Lp].mean()), thresh / 65536.0
            assert abs(kr - (1 - p)) < 5 * math.sqrt(p * (1 - p) / keep[Lp].numel()) + 1e-4, (Lp, kr)
            del bn

    def operand(Lp):
        """u_Lp = round(mask / (1-p) (r s + t)) in the reference's column order (fc1: k = c 12 + w), and its ambiguous steps: the
        kernel forms it in f32 from the same stored r, s, t while staging, and never stores it"""
        if Lp == 1:
            pre = (acts[1].reshape(N, 12, 64) * st[1][2] + st[1][3]).permute(0, 2, 1).reshape(N, 768)
        else:
            pre = acts[Lp] * st[Lp][2] + st[Lp][3]
            if keep[Lp] is not None:
                pre = pre * keep[Lp] * inv_keep
        return rnd(pre), amb(pre, F32_OPS * pre.abs())

    us, ua = {}, {}
    for Lp in range(1, 9):
        us[Lp], ua[Lp] = operand(Lp)
    Wr = {i: rnd(W[f"emg_net.linear.{li}.weight"].double()) for i, li in enumerate(LIN)}
    Wlast = rnd(W["emg_net.last.0.weight"].double())                 # (16, 512)
    for i, li in enumerate(LIN):
        L, Lp = i + 2, i + 1
        b = W[f"emg_net.linear.{li}.bias"].double()
        ref = rnd(torch.relu(us[Lp] @ Wr[i].t() + b))
        allow = ua[Lp] @ Wr[i].abs().t()
        check_act(f"fwd/fc{i + 1}", acts[L], ref, allow=allow)
        moved_enough(f"fwd/fc{i + 1}", ref[-1] - rnd(torch.relu(b)), ref[-1], ref, allow_row=allow[-1])
        check_stats(L, acts[L], N)
    z_ref = us[8] @ Wlast.t()
    allow = ua[8] @ Wlast.abs().t()
    check_param("fwd/proj z", z, z_ref, "wgrad", allow=allow)
    moved_param("fwd/proj z", z_ref[-1], z_ref, "wgrad", allow=allow[-1])
    if not train:
        return

    # ---------------- head: the loss and dz by float64 autograd on the device's own z (the head kernel itself is not under test) ----
    zt = z.detach().double().requires_grad_(True)
    E = W["glove_net.easy.0.weight"].double().t() + W["glove_net.easy.0.bias"].double()
    zn = zt / zt.norm(dim=-1, keepdim=True)
    logits = zn.reshape(B, T, 16) @ (E / E.norm(dim=-1, keepdim=True)).t()
    tgt = torch.arange(T, device="cuda").repeat(B)
    loss = (torch.nn.functional.cross_entropy(logits.reshape(-1, T), tgt)
            + torch.nn.functional.cross_entropy(logits.transpose(1, 2).reshape(-1, T), tgt)) / 2
    loss.backward()
    assert out[0].item() == pytest.approx(loss.item(), rel=1e-5)
    dz_all = tap[10].reshape(-1)[:N * 64].reshape(N, 64).double()     # dz as the head stored it: the projection launch's own input
    assert float(dz_all[:, 16:].abs().max()) == 0.0                  # (the launch contracts over 64 columns: 48 of padding)
    dz = dz_all[:, :16]
    # (a sanity check of the INPUT, not of the head: two bf16 steps; f32: the head's bar in recompute_check, 2e-4)
    if bf16:
        check_act("head/dz (stored, against round(autograd))", dz, rnd(zt.grad), steps=2)
    else:
        check_param("head/dz (stored, against autograd)", dz, zt.grad, "head_f32")
    del logits, zn

    # ---------------- backward: the projection launch and fc7..fc1 -------------------------------------------------------------
    twice = bf16 and not ksplit                                      # the tile passes through LDS in bf16 before mask and rounding

    def slot(L, width=512):
        return tap[L].reshape(-1)[:N * width].reshape(N, width).double()

    def launch(name, A, Aa, L, Wt_r, Lp, dW_got, db_got, next_slot):
        """one launch's outputs from A' (N, F; Aa = its ambiguous steps): dW = A'^T u_Lp, db = sum A', Gout = round(mask / (1-p)
        (A' round(W))) -> next_slot"""
        u = us[Lp]
        dW = A.t() @ u
        allow = Aa.t() @ u.abs() + A.abs().t() @ ua[Lp]
        check_param(f"bwd/{name} dW", dW_got, dW, "wgrad", allow=allow)
        moved_param(f"bwd/{name} dW", A[-1][:, None] * u[-1][None, :], dW, "wgrad", allow=allow)
        if db_got is not None:
            db = A.sum(0)
            check_param(f"bwd/{name} db", db_got, db, "bgrad", allow=Aa.sum(0))
            moved_param(f"bwd/{name} db", A[-1], db, "bgrad", allow=Aa.sum(0))
        acc, allow = A @ Wt_r, Aa @ Wt_r.abs()                       # (N, K), the reference's column order
        if twice:
            acc = rnd(acc)
        if keep[Lp] is not None:
            acc, allow = acc * keep[Lp] * inv_keep, allow * keep[Lp] * inv_keep
        if Lp == 1:
            acc, allow = (t.reshape(N, 64, 12).permute(0, 2, 1).reshape(N, 768) for t in (acc, allow))       # -> [w][c]
        gout = rnd(acc)
        steps = 2 if (twice and keep[Lp] is not None) else 1
        check_act(f"bwd/{name} Gout -> slot {next_slot}", slot(next_slot, gout.shape[1]), gout, steps=steps, allow=allow)
        moved_enough(f"bwd/{name} Gout", gout[-1], gout[-1], gout, steps=steps, allow_row=allow[-1])

    launch("proj", dz, torch.zeros_like(dz), None, Wlast, 8, G["emg_net.last.0.weight"], None, 8)
    for L in range(8, 1, -1):
        i, Lp = L - 2, L - 1
        li = LIN[i]
        gin, r = slot(L), acts[L]
        mean, invstd, scl = st[L][0], st[L][1], st[L][2]
        s1, s2 = gin.sum(0), (gin * r).sum(0)
        dot = (s2 - mean * s1) * invstd
        check_param(f"bwd/bn{L} gamma", G[bnn[L] + ".weight"], dot, "bn")
        check_param(f"bwd/bn{L} beta", G[bnn[L] + ".bias"], s1, "bn")
        c1, c2 = s1 / N, dot / N
        ca, cb, cz = (t.float().double() for t in (scl, -scl * invstd * c2, -scl * (c1 - mean * invstd * c2)))
        pre = (r > 0) * (ca * gin + cb * r + cz)
        # how far the device's f32 value of an element can be from `pre`: its fma chain, and its coefficients -- the launch derives
        # them from ITS totals and writes those out as dgamma and dbeta (f32), so the distance to this reference's sums is observed
        # (d_dot and d_s1 are outputs of the launch under test: this is safe only because the two check_param(..., "bn") calls above
        #  have ALREADY held them to 3e-6 of their maximum -- keep those assertions in front of these lines)
        d_dot = (G[bnn[L] + ".weight"].double() - dot).abs() + 2.0 ** -24 * dot.abs()
        d_s1 = (G[bnn[L] + ".bias"].double() - s1).abs() + 2.0 ** -24 * s1.abs()
        d_cb, d_cz = scl.abs() * invstd * d_dot / N, scl.abs() * (d_s1 / N + mean.abs() * invstd * d_dot / N)
        delta = F32_OPS * ((ca * gin).abs() + (cb * r).abs() + cz.abs()) + d_cb * r.abs() + d_cz
        A, Aa = rnd(pre), amb(pre, delta)
        del pre, delta
        launch(f"fc{i + 1}", A, Aa, L, Wr[i], Lp, G[f"emg_net.linear.{li}.weight"], G[f"emg_net.linear.{li}.bias"], 9 if Lp == 1 else Lp)
        del gin, A

    # ---------------- backward: the conv tail --------------------------------------------------------------------------------
    g9, r2 = slot(9, 768).reshape(N * 12, 64), r1.reshape(N * 12, 64)
    mean, invstd, scl = st[1][0], st[1][1], st[1][2]
    s1, s2 = g9.sum(0), (g9 * r2).sum(0)
    dot = (s2 - mean * s1) * invstd
    check_param("bwd/bn1 gamma (conv2's BatchNorm, from fc1's partial rows)", G[bnn[1] + ".weight"], dot, "bn")
    check_param("bwd/bn1 beta", G[bnn[1] + ".bias"], s1, "bn")
    c1, c2 = s1 / (N * 12), dot / (N * 12)
    ca, cb, cz = (t.float().double() for t in (scl, -scl * invstd * c2, -scl * (c1 - mean * invstd * c2)))
    g2 = slot(1, 768).reshape(N, 12, 64)                             # dL/d(conv2 pre-activation), written over slot 9's tensor
    check_act("bwd/conv2_wgrad: BatchNorm2 + ReLU backward in place, slot 9 -> slot 1", g2.reshape(N * 12, 64), rnd((r2 > 0) * (ca * g9 + cb * r2 + cz)))
    check_param("bwd/conv2 db", G["emg_net.conv_emg.3.bias"], g2.reshape(-1, 64).sum(0), "bgrad")
    dwc2 = torch.zeros(64, 64, 3, 3, dtype=torch.float64, device="cuda")
    for t in range(3):                                               # the raw product with r0, BatchNorm1's affine applied to the result: u1 unrounded
        dwc2[:, :, 1, t] = g2.reshape(-1, 64).t() @ _shift_w(u1x, t - 1).reshape(-1, 64)
    check_param("bwd/conv2 dW", G["emg_net.conv_emg.3.weight"], dwc2, "wgrad")
    assert float(G["emg_net.conv_emg.3.weight"][:, :, 0, :].abs().max()) == 0.0      # rows 0 and 2 only ever meet padding
    assert float(G["emg_net.conv_emg.3.weight"][:, :, 2, :].abs().max()) == 0.0
    gu1 = sum(_shift_w(g2, 1 - t) @ wc2r[:, :, t] for t in range(3))              # conv2's data gradient (N, 12, 64), f32 in the accumulators
    check_act("bwd/conv2 dgrad (stand-alone launch) -> slot 0", slot(0, 768).reshape(N, 12, 64), rnd(gu1))
    gu1, r0f = gu1.reshape(N * 12, 64), r0.reshape(N * 12, 64)
    mean, invstd, scl = st[0][0], st[0][1], st[0][2]
    s1, s2 = gu1.sum(0), (gu1 * r0f).sum(0)
    dot = (s2 - mean * s1) * invstd
    check_param("bwd/bn0 gamma (from conv2's weight-gradient product)", G[bnn[0] + ".weight"], dot, "bn")
    check_param("bwd/bn0 beta", G[bnn[0] + ".bias"], s1, "bn")
    c1, c2 = s1 / (N * 12), dot / (N * 12)
    ca, cb, cz = (t.float().double() for t in (scl, -scl * invstd * c2, -scl * (c1 - mean * invstd * c2)))
    g0 = ((r0f > 0) * (ca * gu1 + cb * r0f + cz)).reshape(N, 12, 64)           # consumed in the accumulators: never rounded
    check_param("bwd/conv1 db", G["emg_net.conv_emg.0.bias"], g0.reshape(-1, 64).sum(0), "bgrad")
    dw1 = torch.stack([(g0 * xp[:, t:t + 12].unsqueeze(-1)).reshape(-1, 64).sum(0) for t in range(3)], -1)   # (64, 3)
    check_param("bwd/conv1 dW", G["emg_net.conv_emg.0.weight"][:, 0, 1, :], dw1, "wgrad")
    assert float(G["emg_net.conv_emg.0.weight"][:, 0, 0, :].abs().max()) == 0.0
    assert float(G["emg_net.conv_emg.0.weight"][:, 0, 2, :].abs().max()) == 0.0


SUMMARY_COLUMNS = ("fwd act", "fwd act identical", "Gout", "Gout identical", "rms", "z", "dW", "db", "gamma/beta",
                   "dW where a rounding is ambiguous", "error/(bar + allowance)", "guard")


def _print(report, groups, N, dtype, adabn, dp, train):
    """the per-launch lines, then ONE line of the case's worst figures: the rows of the table in the module docstring and in DESIGN.md
    7e-2 are these lines, copied"""
    head = f"{dtype}, {'AdaBN' if adabn else 'stock BN'}, dp {dp}, {groups} groups = {N} rows, {'training step' if train else 'evaluation, forward only'}"
    print(f"\nsmall-batch path, launch by launch ({head}; plan {host_plan(N)[1:]}):")
    for k, v in report.items():
        if k != SUMMARY:
            print("  %-78s %s" % (k, v))
    fig = report.get(SUMMARY, {})
    print("  summary (%s): " % head + " | ".join("%s %s" % (c, ("%.5f" if "identical" in c else "%.2g") % fig[c] if c in fig else "-") for c in SUMMARY_COLUMNS))


@pytest.mark.parametrize("dp", [0.0, P_DROP])
@pytest.mark.parametrize("groups", sorted(TABLE))
def test_bf16_stock_bn_step_launch_by_launch(groups, dp):
    small_recompute_check(groups, "bf16", False, dp)


@pytest.mark.parametrize("groups", [7, 25])
def test_bf16_adabn_step_launch_by_launch(groups):
    small_recompute_check(groups, "bf16", True, P_DROP)


@pytest.mark.parametrize("groups", [1, 25])
def test_f32_step_launch_by_launch(groups):
    small_recompute_check(groups, "f32", False, P_DROP)


def test_bf16_adabn_evaluation_takes_the_small_forward():
    """evaluation under AdaBN normalises with batch statistics, so up to 2,624 windows it runs the small forward: 25 groups x 2
    samples = 2,050 windows, forward checks only"""
    small_recompute_check(50, "bf16", True, P_DROP, train=False)
