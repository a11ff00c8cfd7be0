"""The float64 references and the operand recipes that tests/test_gpu_bn_exact.py and tests/test_bn_reference_host.py share (a
helper, not a test module): BatchNorm statistics and backward coefficients from partial rows, the streaming passes around them, the
weight-preparation layouts, the dropout keep decision, the exact-tier partial rows and the float32 error bounds of the real-valued tier.
Everything takes and returns torch tensors on the device of its inputs; float64 unless said otherwise."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24             # a correctly rounded float32 operation errs by at most U32 * |result| (half an ulp, relative form)
E64 = 2.0 ** -53             # the same for float64
SQRT_ULPS = 1.0              # charged to sqrtf and to the float division each: one ulp, i.e. 2 * U32 relative (no figure for either is
DIV_ULPS = 1.0               # in the ROCm headers or documents at hand; a correctly rounded one would be 0.5)
REDUCE_SLICES = 32
FIN_DIRECT_ROWS = 2048
DP_THRESH, DP_INV_KEEP, DP_KEY = 32768, 2.0, 0x5EED1234           # p = 0.5: round(p * 65536), 1 / (1 - 32768 / 65536)


# ---- BatchNorm forward: partial rows -> statistics ------------------------------------------------------------------------------------
def ref_bn_stats(rows, count, gamma, beta, eps, unscale_exp=0):
    """rows[n][2][C] (sum, sum of squares; any floating type, taken to float64) -> dict of float64 [C] vectors: mean, var (biased,
    clamped at 0), unbiased (var count / (count - 1); count == 1: var), invstd = 1 / sqrt(var + eps), scale = gamma invstd,
    shift = beta - mean scale.  unscale_exp: the sums are of values stored times 2^e."""
    r = rows.double()
    s1 = r[:, 0].sum(0) * 2.0 ** -unscale_exp
    s2 = r[:, 1].sum(0) * 2.0 ** (-2 * unscale_exp)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    unbiased = var * count / (count - 1) if count > 1 else var.clone()
    invstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    scale = gamma.double() * invstd
    return dict(mean=mean, var=var, unbiased=unbiased, invstd=invstd, scale=scale, shift=beta.double() - mean * scale)


def ref_running(old, batch, momentum):
    """the momentum convention: new = (1 - m) old + m batch (batch: the mean, or the UNBIASED variance)"""
    return (1.0 - momentum) * old.double() + momentum * batch.double()


def ref_running_stats(mean, var, gamma, beta, eps):
    """evaluation with the running statistics -> [4][C] = mean, invstd, scale, shift"""
    invstd = 1.0 / torch.sqrt(var.double() + float(np.float32(eps)))
    scale = gamma.double() * invstd
    return torch.stack([mean.double(), invstd, scale, beta.double() - mean.double() * scale])


# ---- BatchNorm backward: partial rows -> coefficients ---------------------------------------------------------------------------------
def fold_sums(rows, C, nfold):
    """rows[n][2][C nfold], feature f C + c belonging to channel c -> (sum g, sum g r) per channel"""
    r = rows.double().reshape(rows.shape[0], 2, nfold, C)
    return r[:, 0].sum((0, 1)), r[:, 1].sum((0, 1))


def ref_bn_bwd_coef(rows, count, mean, invstd, scale, C, nfold=1, local=None):
    """g_y = [r > 0] (ca g + cb r + cz) with g the gradient into the BatchNorm's OUTPUT and r its input:
        x_hat = (r - mean) invstd,  dgamma = sum g x_hat,  dbeta = sum g,  g_r = scale (g - mean(g) - x_hat mean(g x_hat))
    local (one row [2][C nfold]): coef from `rows` and `count`, dgamma / dbeta from `local`."""
    mean, invstd, scale = mean.double(), invstd.double(), scale.double()
    s1, s2 = fold_sums(rows, C, nfold)
    dot = (s2 - mean * s1) * invstd
    c1, c2 = s1 / count, dot / count
    coef = torch.stack([scale, -scale * invstd * c2, -scale * (c1 - mean * invstd * c2)])
    if local is not None:
        l1, l2 = fold_sums(local.reshape(1, 2, C * nfold), C, nfold)
        return dict(coef=coef, dgamma=(l2 - mean * l1) * invstd, dbeta=l1, s1=s1, s2=s2)
    return dict(coef=coef, dgamma=dot, dbeta=s1, s1=s1, s2=s2)


def ref_bn_relu_bwd(g, r, coef):
    ca, cb, cz = (c.double() for c in coef)
    g, r = g.double(), r.double()
    return torch.where(r > 0, ca * g + cb * r + cz, torch.zeros_like(g))


def ref_dropout_apply(r, scale, shift, keep, inv_keep):
    r = r.double()
    return torch.where(keep, (scale.double() * r + shift.double()) * inv_keep, torch.zeros_like(r))


# ---- the dropout hash ------------------------------------------------------------------------------------------------------------------
def keep_mask(key, M, thresh, ld=512):
    """the kernels' keep decision for element (m, f) of an [M][ld] tensor, from the numpy restatement of csrc/common.cuh dropout_quad
    (tools/dropout_hash_check.py): quad index (m * ld + f) >> 2, draw f & 3.  A numpy bool array."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dropout_hash_check as dh
    q = ld // 4
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(q) + np.arange(q, dtype=np.uint64)[None, :]
    a, b = dh.quad(idx, np.uint64(key))
    return np.stack(dh.draws(a, b), axis=-1).reshape(M, ld) >= thresh


def kept_share_ok(keep, M):
    """the kept share of the first M rows lies within 6 binomial standard deviations of 0.5"""
    n = M * keep.shape[1]
    share = float(keep[:M].sum()) / n
    return abs(share - 0.5) <= 6 * (0.25 / n) ** 0.5, share


# ---- weight preparation ----------------------------------------------------------------------------------------------------------------
def ref_fold(W, b, s, t, mode, rows_out=None):
    """y = (r s + t) W^T + b = r (W diag s)^T + (b + W t).  W (F, K); mode 0: channel = k, stored k' = k; mode 1 (K = 768): source
    k = c * 12 + w, channel c, stored k' = w * 64 + c.  s / t None: the plain copy.  Returns the image [rows_out][K] (rows >= F zero)
    and the bias [F] (b None: 0), float64."""
    F, K = W.shape
    W = W.double()
    ch = torch.arange(K, device=W.device) // 12 if mode == 1 else torch.arange(K, device=W.device)
    sk = s.double()[ch] if s is not None else torch.ones(K, dtype=torch.float64, device=W.device)
    img = W * sk
    if mode == 1:
        img = img.reshape(F, 64, 12).permute(0, 2, 1).reshape(F, K)
    bias = torch.zeros(F, dtype=torch.float64, device=W.device) if b is None else b.double().clone()
    if t is not None:
        bias = bias + W @ t.double()[ch]
    if rows_out is not None and rows_out > F:
        img = torch.cat([img, torch.zeros(rows_out - F, K, dtype=torch.float64, device=W.device)])
    return img.contiguous(), bias


def ref_transpose(W, mode, ld_out):
    """out[k'][j] = W[j][k], columns j >= F zero; mode 1: k' = (k % 12) * 64 + k / 12"""
    F, K = W.shape
    W = W.double()
    out = W.reshape(F, 64, 12).permute(2, 1, 0).reshape(K, F) if mode == 1 else W.T
    if ld_out > F:
        out = torch.cat([out, torch.zeros(K, ld_out - F, dtype=torch.float64, device=W.device)], 1)
    return out.contiguous()


def coded_w1(device, bf16):
    """a (512, 768) weight whose entry encodes its place in the conv stack: W[j][c * 12 + w] = (-1)^j (1 + c + 64 w), an integer of at
    most 768; for bf16 images (-1)^j (1 + c % 16 + 16 w) <= 192, which has eight significant bits and so is a bf16 number.  A swapped
    k / 12 and k % 12 moves every entry to a place that expects another code."""
    j = torch.arange(512, device=device)[:, None, None]
    c = torch.arange(64, device=device)[None, :, None]
    w = torch.arange(12, device=device)[None, None, :]
    code = (1 + c % 16 + 16 * w) if bf16 else (1 + c + 64 * w)
    return ((1 - 2 * (j % 2)) * code).reshape(512, 768).float().contiguous()


def ternary(shape, gen, n, device):
    """1 and -1 with probability 1 / n each, else 0"""
    u = torch.randint(0, n, shape, generator=gen, device=device)
    return (u == 0).float() - (u == 1).float()


def prep_weights(device):
    """the weights the preparation launches read, exact by construction: W1 (512, 768), W2..W7 (512, 512) and Wp (16, 512) ternary
    (-1 / 1 with probability 1/4 each), b1..b7 integers in -3..3"""
    gen = torch.Generator(device=device).manual_seed(70212)
    o = {}
    for i in range(7):
        o["W%d" % (i + 1)] = ternary((512, 768 if i == 0 else 512), gen, 4, device).contiguous()
        o["b%d" % (i + 1)] = torch.randint(-3, 4, (512,), generator=gen, device=device).float()
    o["Wp"] = ternary((16, 512), gen, 4, device).contiguous()
    return o


# ---- the pre-reduce, as reduce_rows_kernel adds (float32) ----------------------------------------------------------------------------------
def reduce_rows_f32(rows):
    """rows[n][W] float32 -> [32][W] float32 in reduce_rows_kernel's own order of float32 additions: row r belongs to slice r % 32 and,
    within it, to lane g = (r / 32) % 4; a lane adds its rows in ascending order starting from 0, and the slice is
    ((lane 0 + lane 1) + lane 2) + lane 3."""
    n, W = rows.shape
    assert rows.dtype == torch.float32
    per = -(-n // 128) * 128
    pad = torch.zeros(per, W, dtype=torch.float32, device=rows.device)
    pad[:n] = rows
    pad = pad.reshape(per // 128, 4, REDUCE_SLICES, W)              # [j][g][slice]: row = slice + 32 g + 128 j
    live = (torch.arange(per, device=rows.device) < n).reshape(per // 128, 4, REDUCE_SLICES, 1)
    acc = torch.zeros(4, REDUCE_SLICES, W, dtype=torch.float32, device=rows.device)
    for j in range(per // 128):
        acc = torch.where(live[j], acc + pad[j], acc)              # (a row past n is not added at all: -0 + 0 aside, the same thing)
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def reduce_rows_bound(rows):
    """|float32 slice sum - exact slice sum| <= (adds in the longest chain) U32 sum |x| over the slice, first order, times 1 + 2^-10
    for the higher orders: each of a chain's additions rounds a partial sum that is at most sum |x| in magnitude."""
    n, W = rows.shape
    per = -(-n // 128) * 128
    pad = torch.zeros(per, W, dtype=torch.float64, device=rows.device)
    pad[:n] = rows.double()
    pad = pad.reshape(per // 128, 4, REDUCE_SLICES, W)
    exact = pad.sum((0, 1))
    depth = per // 128 + 3
    return exact, depth * U32 * (1 + 2.0 ** -10) * pad.abs().sum((0, 1))


def rows_as_finalized(rows):
    """what the finalize kernel is handed: the rows themselves up to FIN_DIRECT_ROWS of them, else the 32 float32 rows of the pre-reduce"""
    n = rows.shape[0]
    if n <= FIN_DIRECT_ROWS:
        return rows
    return reduce_rows_f32(rows.reshape(n, -1)).reshape((REDUCE_SLICES,) + tuple(rows.shape[1:]))


# ---- the exact tier: partial rows with planted totals ---------------------------------------------------------------------------------------
def spread_totals(totals, n, gen, step=1.0, span=500):
    """n rows of multiples of `step` whose column sums are `totals` (float64, multiples of step): random rows in [-span, span] steps,
    the last row takes the rest.  Returns float32 [n][len(totals)]; asserts that every entry is a float32 number and that sum |x| stays
    below 2^24 steps, so that every float32 or float64 sum of these rows, in any order and grouping, is exact."""
    W = totals.numel()
    q = torch.round(totals.double() / step)
    assert torch.equal(q * step, totals.double()), "totals are not multiples of the step"
    body = torch.randint(-span, span + 1, (n - 1, W), generator=gen, device=totals.device).double()
    rows = torch.cat([body, (q - body.sum(0))[None]])
    assert float(rows.abs().sum(0).max()) < 2 ** 24, "sum |x| reaches 2^24 steps"
    out = (rows * step).float()
    assert torch.equal(out.double().sum(0), totals.double())
    return out


def plant_forward_totals(C, count, gen, device, unscale_exp=0, small=False):
    """per column: mean = p / 4, unbiased variance U = q (an integer >= 1), var = q (count - 1) / count; count a power of two (or 1:
    var = q).  One column (index 1) has s2 / count = mean^2 - 1 < mean^2: the clamp.  Returns the totals (s1, s2) in STORED units
    (times 2^e, 4^e) and the float64 mean / var / unbiased they stand for; every quantity is exactly representable (asserted)."""
    pr, qr = (8, 4) if small else (32, 16)
    p = torch.randint(-pr, pr + 1, (C,), generator=gen, device=device).double()
    p[1] = 3.0
    q = torch.randint(1, qr + 1, (C,), generator=gen, device=device).double()
    mean = p / 4
    if count > 1:
        assert count & (count - 1) == 0, "count must be a power of two"
        var = q * (count - 1) / count
    else:
        var = q.clone()
    ex2 = var + mean * mean
    ex2[1] = mean[1] * mean[1] - 1.0
    var[1] = 0.0
    unbiased = torch.where(var > 0, q, torch.zeros_like(q))
    s1, s2 = mean * count, ex2 * count
    for name, v in (("mean", mean), ("var", var), ("E[x^2]", ex2), ("unbiased", unbiased)):
        assert torch.equal(v, v.float().double()), "%s is not a float32 number" % name
    assert torch.equal(s2 / count - mean * mean, torch.where(var > 0, var, -torch.ones_like(var))), "s2 / count - mean^2 is not exact"
    if count > 1:
        assert torch.equal(var * count / (count - 1), unbiased), "var count / (count - 1) is not exact"
    return dict(s1=s1 * 2.0 ** unscale_exp, s2=s2 * 4.0 ** unscale_exp, mean=mean, var=var, unbiased=unbiased)


# ---- the real-valued tier: float32 error bounds --------------------------------------------------------------------------------------------
def stats_bounds(rows, count, ref, gamma, beta, eps, unscale_exp=0):
    """Absolute error bounds of bn_finalize_kernel's four outputs against ref = ref_bn_stats(rows, ...), rows being what the kernel is
    handed.  The kernel sums in float64 and forms mean and var in float64, then

        mean   = (float) mu                        one rounding:                                  U32 |mu|
        var    = (float) vb                        one rounding:                                  U32 relative
        x      = var + eps                         one float32 addition:                          U32 relative    (var, eps >= 0: no cancellation)
        r      = sqrtf(x)                          SQRT_ULPS ulps = 2 SQRT_ULPS U32 relative, and half of x's relative error
        invstd = 1.0f / r                          DIV_ULPS ulps  = 2 DIV_ULPS U32 relative, and r's relative error
        scale  = gamma * invstd                    one multiplication:                            U32 relative, and invstd's
        shift  = beta - mean * scale               a multiplication and a subtraction, or one fma: U32 |mean scale| + U32 |shift| covers both,
                                                   and the product carries mean's and scale's relative errors

    so invstd errs by (1 + 2 SQRT_ULPS + 2 DIV_ULPS) U32 relative plus half of d64 / (var + eps), d64 being the float64 part: the
    rounding of the n + 2 float64 additions and the division behind each of s1 / count and s2 / count, of the product mu * mu and of
    the subtraction, which cancellation magnifies where |mean| / std is large -- it is bounded with sum |x| in place of |sum x|.
    Every bound is multiplied by 1 + 2^-10 for the higher-order terms."""
    r = rows.double()
    n = r.shape[0]
    a1 = r[:, 0].abs().sum(0) * 2.0 ** -unscale_exp / count
    a2 = r[:, 1].abs().sum(0) * 2.0 ** (-2 * unscale_exp) / count
    mu = ref["mean"]
    d_mu = 2 * (n + 2) * E64 * a1                    # (twice: the reference's own float64 sums err as much)
    d64 = 2 * (n + 2) * E64 * a2 + 2 * mu.abs() * d_mu + 3 * E64 * (a2 + mu * mu)
    x = ref["var"] + float(np.float32(eps))
    slack = 1 + 2.0 ** -10
    rel_inv = (1 + 2 * SQRT_ULPS + 2 * DIV_ULPS) * U32 + 0.5 * d64 / x
    rel_scale = rel_inv + U32
    e_mean = U32 * mu.abs() + d_mu
    prod = (mu * ref["scale"]).abs()
    e_shift = prod * (rel_scale + U32) + ref["scale"].abs() * e_mean + U32 * ref["shift"].abs()
    return dict(mean=e_mean * slack, invstd=rel_inv * ref["invstd"].abs() * slack, scale=rel_scale * ref["scale"].abs() * slack,
                shift=e_shift * slack)


def running_stats_bounds(table):
    """the same chain from a float32 var (bn_running_stats_kernel): x = var + eps U32, sqrtf, division, product; mean is copied"""
    mean, invstd, scale, shift = table
    slack = 1 + 2.0 ** -10
    rel_inv = (0.5 + 2 * SQRT_ULPS + 2 * DIV_ULPS) * U32
    rel_scale = rel_inv + U32
    prod = (mean * scale).abs()
    return torch.stack([torch.zeros_like(mean), rel_inv * invstd.abs() * slack, rel_scale * scale.abs() * slack,
                        (prod * (rel_scale + U32) + U32 * shift.abs()) * slack])


def coef_bounds(rows, count, mean, invstd, scale, C, nfold, ref, local=None):
    """Absolute error bounds of bn_bwd_finalize_kernel's outputs: each is ONE float32 rounding (U32 relative) of a float64 expression,
    whose own error d64 is bounded term by term with sums of magnitudes in place of the sums (n nfold + 2 additions each; the
    subtractions s2 - mean s1 and c1 - mean invstd c2 may cancel):
        d(s1) = k E64 A1, d(s2) = k E64 A2,  k = n nfold + 2,  A = sum of magnitudes
        d(dot) = invstd (d(s2) + |mean| d(s1) + 3 E64 (A2 + |mean| A1))
        d(cb)  = |scale invstd| d(dot) / count + 4 E64 |cb|
        d(cz)  = |scale| (d(s1) / count + |mean invstd| d(dot) / count + 6 E64 (|c1| + |mean invstd c2|))"""
    def mags(r):
        r = r.double().reshape(-1, 2, nfold, C).abs()
        return r[:, 0].sum((0, 1)), r[:, 1].sum((0, 1)), 2 * (r.shape[0] * nfold + 2)      # (twice: the reference's own sums err as much)
    mean, invstd, scale = mean.double().abs(), invstd.double().abs(), scale.double().abs()
    A1, A2, k = mags(rows)
    d1, d2 = k * E64 * A1, k * E64 * A2
    ddot = invstd * (d2 + mean * d1 + 3 * E64 * (A2 + mean * A1))
    c1, c2 = ref["s1"].abs() / count, (A2 + mean * A1) * invstd / count
    cb, cz = ref["coef"][1].abs(), ref["coef"][2].abs()
    dcb = scale * invstd * ddot / count + 4 * E64 * cb
    dcz = scale * (d1 / count + mean * invstd * ddot / count + 6 * E64 * (c1 + mean * invstd * c2))
    if local is not None:
        A1, A2, k = mags(local)
        d1, d2 = k * E64 * A1, k * E64 * A2
        ddot = invstd * (d2 + mean * d1 + 3 * E64 * (A2 + mean * A1))
    slack = 1 + 2.0 ** -10
    f32 = lambda ref_v, d: (U32 * (ref_v.abs() + d) + d) * slack
    return dict(coef=torch.stack([torch.zeros_like(cb), f32(ref["coef"][1], dcb), f32(ref["coef"][2], dcz)]),
                dgamma=f32(ref["dgamma"], ddot), dbeta=f32(ref["dbeta"], d1))
