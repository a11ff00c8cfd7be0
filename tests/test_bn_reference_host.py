"""The float64 references of tests/test_gpu_bn_exact.py (tests/bn_reference.py) against torch itself, on the CPU: they are what the
BatchNorm kernels are held to, so they are anchored here -- the forward reference to torch.nn.BatchNorm1d in training mode over two
consecutive batches (momentum, running buffers, unbiased variance), the backward reference to autograd through BatchNorm1d(relu(.))
and, for nfold = 12, BatchNorm2d over a (N, 64, 1, 12) tensor held in the internal [w][c] order; then the recipes' own preconditions:
the exactness of the planted statistics, the kept share of the dropout mask at every row count the GPU module uses, every column of the
ternary weights non-zero, the float32 restatement of the pre-reduce within its derived bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as br  # noqa: E402  (tests/bn_reference.py)


def _partial_rows(x, cuts, second=None):
    """[n][2][C]: (sum x, sum x^2) -- or (sum x, sum x * second) -- over the row ranges between `cuts`"""
    y = x * x if second is None else x * second
    edges = [0] + list(cuts) + [x.shape[0]]
    return torch.stack([torch.stack([x[a:b].sum(0), y[a:b].sum(0)]) for a, b in zip(edges[:-1], edges[1:])])


def _close(got, ref, rel=1e-12):
    assert float((got - ref).abs().max()) <= rel * float(ref.abs().max()), float((got - ref).abs().max())


def test_forward_reference_is_batchnorm1d_in_training_mode():
    """two consecutive batches: the normalisation with the biased variance, the running buffers with momentum and the unbiased one"""
    gen = torch.Generator().manual_seed(11)
    C, eps, momentum = 64, 1e-5, 0.25
    bn = torch.nn.BatchNorm1d(C, eps=float(torch.tensor(eps, dtype=torch.float32)), momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=gen).double() + 0.5)
        bn.bias.copy_(torch.randn(C, generator=gen).double())
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for N, cuts in ((37, (5, 6, 30)), (128, (64,))):
        x = (torch.randn(N, C, generator=gen) * 3 + torch.randn(C, generator=gen) * 5).double()
        y = bn(x)
        ref = br.ref_bn_stats(_partial_rows(x, cuts), N, bn.weight.detach(), bn.bias.detach(), eps)
        _close(x * ref["scale"] + ref["shift"], y.detach())
        _close((x - ref["mean"]) * ref["invstd"] * bn.weight.detach() + bn.bias.detach(), y.detach())
        rm, rv = br.ref_running(rm, ref["mean"], momentum), br.ref_running(rv, ref["unbiased"], momentum)
        _close(rm, bn.running_mean)
        _close(rv, bn.running_var)
    # count == 1: the unbiased variance is the biased one; s2 / count < mean^2: the clamp
    one = br.ref_bn_stats(torch.tensor([[[3.0, -2.0], [10.0, 3.0]]]), 1, torch.ones(2), torch.zeros(2), eps)
    assert one["var"].tolist() == [1.0, 0.0] and one["unbiased"].tolist() == [1.0, 0.0]
    assert float(one["invstd"][1]) == float(1.0 / torch.sqrt(torch.tensor(eps, dtype=torch.float32).double()))
    # unscale_exp: the rows hold sums of values stored times 2^e
    x = torch.randn(9, 4, generator=gen).double()
    a = br.ref_bn_stats(_partial_rows(x, (4,)), 9, torch.ones(4), torch.zeros(4), eps)
    b = br.ref_bn_stats(_partial_rows(x * 8, (4,)), 9, torch.ones(4), torch.zeros(4), eps, unscale_exp=3)
    _close(b["mean"], a["mean"])
    _close(b["var"], a["var"])


def _autograd_case(gen, N, C, nfold):
    """y -> r = relu(y) -> BatchNorm -> sum(v G): the references' inputs (sum g, sum g r; g = G), and what autograd says"""
    eps = 1e-5
    gamma = torch.rand(C, generator=gen).double() + 0.5              # a gamma-scale != 1
    beta = torch.randn(C, generator=gen).double()
    y = torch.randn(N, nfold, C, generator=gen).double().requires_grad_()          # the internal order [w][c]
    G = torch.randn(N, nfold, C, generator=gen).double()
    r = torch.relu(y)
    if nfold == 1:
        bn = torch.nn.BatchNorm1d(C, eps=float(torch.tensor(eps, dtype=torch.float32))).double().train()
        feed = lambda t: t[:, 0]
        back = lambda t: t[:, None]
    else:
        bn = torch.nn.BatchNorm2d(C, eps=float(torch.tensor(eps, dtype=torch.float32))).double().train()
        feed = lambda t: t.permute(0, 2, 1)[:, :, None, :]           # (N, 64, 1, 12): x[n][c][0][w] = r[n][w][c]
        back = lambda t: t[:, :, 0, :].permute(0, 2, 1)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    v = back(bn(feed(r)))
    (v * G).sum().backward()
    rd, Gd = r.detach().reshape(N, nfold * C), G.reshape(N, nfold * C)
    fwd = br.ref_bn_stats(_partial_rows(rd.reshape(N * nfold, C), (N,)), N * nfold, gamma, beta, eps)
    return dict(r=rd, G=Gd, fwd=fwd, gy=y.grad.reshape(N, nfold * C), dgamma=bn.weight.grad, dbeta=bn.bias.grad)


@pytest.mark.parametrize("C,nfold", [(512, 1), (64, 1), (64, 12)])
def test_backward_reference_is_autograd_through_batchnorm_of_relu(C, nfold):
    gen = torch.Generator().manual_seed(100 + C + nfold)
    N = 23
    a = _autograd_case(gen, N, C, nfold)
    rows = _partial_rows(a["G"], (7, 8), second=a["r"])                       # [3][2][C nfold]
    f = a["fwd"]
    ref = br.ref_bn_bwd_coef(rows, N * nfold, f["mean"], f["invstd"], f["scale"], C, nfold)
    _close(ref["dgamma"], a["dgamma"])
    _close(ref["dbeta"], a["dbeta"])
    coef = ref["coef"].repeat(1, nfold)                                         # feature f C + c has channel c's coefficients
    _close(br.ref_bn_relu_bwd(a["G"], a["r"], coef), a["gy"])
    # `local`: the coefficients from `rows` and the global count, dgamma / dbeta from the local row alone
    local = rows[1]
    both = br.ref_bn_bwd_coef(rows, N * nfold, f["mean"], f["invstd"], f["scale"], C, nfold, local=local)
    alone = br.ref_bn_bwd_coef(rows[1:2], N * nfold, f["mean"], f["invstd"], f["scale"], C, nfold)
    assert torch.equal(both["coef"], ref["coef"])
    assert torch.equal(both["dgamma"], alone["dgamma"]) and torch.equal(both["dbeta"], alone["dbeta"])


def test_fold_and_transpose_references_state_the_layer():
    """y = (r s + t) W^T + b with r in the internal order equals r' (image)^T + bias, for both modes; the transpose undoes the order"""
    gen = torch.Generator().manual_seed(5)
    for mode, K, C in ((0, 512, 512), (1, 768, 64)):
        W = torch.randn(512, K, generator=gen).double()
        b, s, t = torch.randn(512, generator=gen).double(), torch.rand(C, generator=gen).double() + 0.5, torch.randn(C, generator=gen).double()
        r = torch.randn(6, K, generator=gen).double()                           # reference order: k = c * 12 + w in mode 1
        ch = torch.arange(K) // 12 if mode == 1 else torch.arange(K)
        want = (r * s[ch] + t[ch]) @ W.T + b
        stored = r.reshape(6, 64, 12).permute(0, 2, 1).reshape(6, K) if mode == 1 else r
        img, bias = br.ref_fold(W, b, s, t, mode)
        _close(stored @ img.T + bias, want)
        g = torch.randn(6, 512, generator=gen).double()
        dg = g @ W                                                              # gradient in the reference order
        dg_stored = dg.reshape(6, 64, 12).permute(0, 2, 1).reshape(6, K) if mode == 1 else dg
        _close(g @ br.ref_transpose(W, mode, 512).T, dg_stored)
    img, bias = br.ref_fold(torch.ones(16, 512), None, None, None, 0, rows_out=32)
    assert img.shape == (32, 512) and not bool(img[16:].any()) and not bool(bias.any())
    assert br.ref_transpose(torch.ones(16, 512), 0, 64).shape == (512, 64)
    for bf16 in (False, True):
        W = br.coded_w1("cpu", bf16)
        assert torch.equal(W, W.bfloat16().float()) or not bf16
        swapped = W.reshape(512, 12, 64).permute(0, 2, 1).reshape(512, 768)       # k / 12 and k % 12 exchanged
        assert not torch.equal(br.ref_fold(W, None, None, None, 1)[0], br.ref_fold(swapped, None, None, None, 1)[0])
        assert float((br.ref_fold(W, None, None, None, 1)[0] != br.ref_fold(swapped, None, None, None, 1)[0]).double().mean()) > 0.9


def test_planted_statistics_are_exact():
    """the exact tier's totals: mean, E[x^2], var and var count / (count - 1) are float32 numbers (asserted inside), the rows sum to
    them in any order, and the float64 reference returns exactly what was planted -- contracted or not"""
    gen = torch.Generator().manual_seed(7)
    for C in (64, 512):
        for count, e, small, step in ((4096, 0, False, 1.0), (4096, 3, True, 1.0), (4096, -2, True, 2.0 ** -8), (1, 0, True, 2.0 ** -8)):
            t = br.plant_forward_totals(C, count, gen, "cpu", unscale_exp=e, small=small)
            for n in (1, 65, 2049):
                rows = br.spread_totals(torch.cat([t["s1"], t["s2"]]), n, gen, step=step).reshape(n, 2, C)
                ref = br.ref_bn_stats(rows, count, torch.ones(C), torch.zeros(C), 1e-5, unscale_exp=e)
                assert torch.equal(ref["mean"], t["mean"]) and torch.equal(ref["var"], t["var"]) and torch.equal(ref["unbiased"], t["unbiased"])
                fed = br.rows_as_finalized(rows)                                # the float32 pre-reduce is exact on these rows
                ref2 = br.ref_bn_stats(fed, count, torch.ones(C), torch.zeros(C), 1e-5, unscale_exp=e)
                assert torch.equal(ref2["mean"], t["mean"]) and torch.equal(ref2["var"], t["var"])
            assert float(t["var"][1]) == 0.0 and float(t["unbiased"][1]) == 0.0            # the clamped column
            # the running update at momentum 1/2 from priors that are multiples of 1/8
            old = torch.randint(-16, 17, (C,), generator=gen).double() / 8
            for batch in (t["mean"], t["unbiased"]):
                new = br.ref_running(old, batch, 0.5)
                assert torch.equal(new, new.float().double())


def test_pre_reduce_restatement_stays_within_its_bound():
    gen = torch.Generator().manual_seed(9)
    for n in (2049, 5000):
        rows = (torch.randn(n, 128, generator=gen) * 50 + 200).float()
        got = br.reduce_rows_f32(rows)
        exact, bound = br.reduce_rows_bound(rows)
        assert got.shape == (32, 128)
        assert bool(((got.double() - exact).abs() <= bound).all())
        assert float((got.double() - exact).abs().max()) > 0                    # (the bound is not vacuous: float32 does round here)
        _close(got.double().sum(0), rows.double().sum(0), rel=1e-5)


def test_dropout_mask_recipe():
    """the kept share at p = 0.5 lies within 6 binomial standard deviations of 0.5 at every row count >= 31 of the GPU module"""
    counts = [2047, 2048, 2049, 4096, 4097, 6145, 8193, 1023, 1024, 1025, 3073]
    keep = br.keep_mask(br.DP_KEY, max(counts), br.DP_THRESH)
    for M in counts:
        ok, share = br.kept_share_ok(keep, M)
        assert ok, (M, share)
    # rows differ from each other, and from the mask of another key
    assert not (keep[0] == keep[1]).all() and not (keep[:64] == br.keep_mask(br.DP_KEY ^ 1, 64, br.DP_THRESH)).all()


def test_ternary_weights_have_no_empty_column():
    o = br.prep_weights("cpu")
    for name, W in o.items():
        if name.startswith("W"):
            assert bool((W != 0).any(0).all()), name
