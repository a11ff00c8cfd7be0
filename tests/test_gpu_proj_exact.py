"""The large-batch launches of the 512 -> 16 projection on their own, one sequence at a time through cp_debug_proj, at tolerance ZERO
and ragged row counts.

What runs (include/cpnative.h, cp_debug_proj; the launch functions are the step's own, csrc/encoder_api.cuh and gemm_ws.cuh):

    kind 0   fold_linear_kernel / the plain copy -> wlast[32][512], blast;  gemm_nt_kernel<T,128,32,.,EPI_PLAIN_F32> -> z[M][16]
             (ALOAD_PLAIN, ALOAD_BNDROP behind a dropout, ALOAD_F8 / ALOAD_BNDROP_F8 on an e4m3 activation)
    kind 1   colsum_kernel + colsum_finalize_kernel -> dzsum;  gemm_tn_kernel<T,64,128,YLOAD_PLAIN | YLOAD_F8> -> slabs[S][64][512];
             reduce_slabs_kernel -> dW, praw;  bn_bwd_sums_from_wgrad_kernel -> one partial row [2][512]
    kind 2   gemm_tn_kernel<T,64,128,YLOAD_BNDROP> + reduce_slabs_kernel -> dW                   (f32 and bf16)
    kind 3   proj_wgrad_sums_kernel<false | true> -> slabs[S][32][512];  proj_wgrad_finish_kernel -> dW, rows[4][2][512]   (bf16)
    kind 4   transpose_w_kernel -> wlast_t[512][64];  proj_dgrad_kernel -> C[M][512], partials[rows][512]                   (bf16)

Why zero (the recipe of tests/test_gpu_fc_gemm_exact.py): dz is ternary (-1 / 1 with probability 1/16 each, else 0; columns 16..63
zero, as the head leaves them), Wp ternary (-1 / 1 with probability 1/4 each: at 1/16 one column in nine of a 16-row matrix never sees
a non-zero weight, asserted below), the saved activation relu(randint(-2, 4)), scale and ca from {0.5, 1, 2}, shift, cb and cz small
integers, dropout at p = 0.5 (threshold 32768, 1 / (1 - p) = 2 exactly), the e4m3 activations the same small integers times
2^r_exp, r_exp in {0, 1, -1}.  Every product, every float32 accumulator, every value a kernel rounds to bf16 and every column sum
then has ONE right answer, whichever block ran which rows and however the sums were grouped.  The reference is the same operation in
float64 torch, and the module asserts these preconditions on that reference before it compares anything (`_exact_values`,
`_exact_stat`, `_exact_acc`); each case prints the largest value and sum it saw (pytest -s).

The mask: the three places that form the dropout decision independently -- bn_drop_chunk in the staging of kinds 0 and 2,
dropout_quad + word_mask in kind 3, dropout_pair in kind 4's epilogue -- are all held to ONE restatement of the hash, numpy's in
tools/dropout_hash_check.py at (key, row, ld = 512, column), so they agree with each other wherever an element reaches an output.
The kept share lies within 6 binomial standard deviations of 0.5.

What is compared (torch.equal): every element of the output below M; the sentinel (a NaN bit pattern) in the guard rows behind M and
in the floats behind the last slab, partial row and prepared weight (z has ldc = 16: a store at f >= 16 lands in the next row, the
last row's in the guard); the slabs summed over S against the raw product; the partial rows summed in float64 against sum g and
sum g r; rows_out against the launcher's formula.

Row counts, the smallest at which each piece of control flow is first taken.  Forward (one block per 128-row tile): 1, 127, 128,
129, 389.  Weight gradients (128 splits, 32-row steps): 1, 31, 32, 33 (S = 2, the second split holds one row), 95 (S = 3), 161
(S = 6: blocks with fy >= splits return, finish-kernel threads see no slab), 1,023 (S = 32), 4,096 (S = 128: the finish kernel's
unrolled walk without a tail), 4,097 (64 rows per split: two steps, the double buffer; S = 65), 8,193 (96 rows, three steps, S = 86)
-- S % 4 = 1, 2, 3, 0 for reduce_slabs_kernel's tail; kind 1 also 16,485 (dz's column sums: the 64-block cap, a block walks more
than one row group; S = 104).  Data gradient (512 blocks = 256 workers x 2 feature halves, 32-row tiles): 1, 31, 32, 33, 8,191,
8,192, 8,193 (one worker's second tile holds one live row: the vmcnt(4) path), 16,485 (a third tile, the buffers wrap).
The operands hold live data behind row M, so a load that lost its row guard shows in the sums."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda" if torch.cuda.is_available() else "cpu"        # (the references run on the CPU too: the recipe against its own preconditions)
F32, BF16 = 0, 1
M_MAX = 16485
M_ALLOC = M_MAX + 160                   # live rows behind the largest M: more than one 128-row tile
GUARD_ROWS = 160                        # behind C: more than one 128-row tile
GUARD_FLOATS = 8192
SENTINEL16 = 0x7FA5                     # a bf16 NaN
SENTINEL32 = 0x7FC0BEEF                 # a float32 NaN
SENTINEL_Z = 0x7FC0CAFE                 # another one for z: a store at f >= 16 adds blast[f], which still holds SENTINEL32, to a zero product
DP_THRESH, DP_INV_KEEP, DP_KEY = 32768, 2.0, 0x5EED1234           # p = 0.5: round(p * 65536), 1 / (1 - 32768 / 65536)
PROJ_SPLITS, PROJ_FINISH_ROWS, PROJ_RT, PROJ_WORKERS = 128, 4, 32, 256

FWD_M = [1, 127, 128, 129, 389]
WGRAD_M = [1, 31, 32, 33, 95, 161, 1023, 4096, 4097, 8193]
DGRAD_M = [1, 31, 32, 33, 8191, 8192, 8193, 16485]
R_EXPS = [None, 0, 1, -1]
_id_exp = lambda e: "plain" if e is None else "e4m3_exp%d" % e
_id_dtype = lambda d: "f32" if d == F32 else "bf16"
TYPES = [(F32, None)] + [(BF16, e) for e in R_EXPS]                # (dtype, r_exp)
TYPE_IDS = ["%s-%s" % (_id_dtype(d), _id_exp(e)) for d, e in TYPES]


# ---- operands --------------------------------------------------------------------------------------------------------------------
def _ternary(shape, gen, n):
    """1 and -1 with probability 1 / n each, else 0"""
    u = torch.randint(0, n, shape, generator=gen, device=DEV)
    return (u == 0).float() - (u == 1).float()


@functools.lru_cache(maxsize=None)
def _operands():
    """the recipe of the module docstring, made once: slices [:M] serve every case"""
    gen = torch.Generator(device=DEV).manual_seed(51216)
    dz = torch.zeros(M_ALLOC, 64, device=DEV)
    dz[:, :16] = _ternary((M_ALLOC, 16), gen, 16)
    Wp = _ternary((16, 512), gen, 4)
    assert bool((Wp != 0).any(0).all()), "a column of Wp never sees a non-zero weight: raise its density"
    R = torch.relu(torch.randint(-2, 4, (M_ALLOC, 512), generator=gen, device=DEV).float())
    pick = torch.tensor([0.5, 1.0, 2.0], device=DEV)
    scale = pick[torch.randint(0, 3, (512,), generator=gen, device=DEV)]
    shift = torch.randint(-2, 3, (512,), generator=gen, device=DEV).float()
    ca = pick[torch.randint(0, 3, (512,), generator=gen, device=DEV)]
    cb = torch.randint(-1, 2, (512,), generator=gen, device=DEV).float()
    cz = torch.randint(-2, 3, (512,), generator=gen, device=DEV).float()
    return dict(dz=dz, Wp=Wp.contiguous(), R=R, scale=scale, shift=shift, coef=torch.stack([ca, cb, cz]).contiguous())


@functools.lru_cache(maxsize=None)
def _typed(name, dtype):
    """dz or R as the kernels read it: T = float or bf16 (the values are bf16 numbers: the conversion is exact)"""
    t = _operands()[name]
    return t.contiguous() if dtype == F32 else t.bfloat16().contiguous()


@functools.lru_cache(maxsize=None)
def _act8(r_exp):
    """R as e4m3 bytes, stored = value * 2^r_exp, and the device word that holds r_exp: exact, asserted"""
    stored = _operands()["R"] * 2.0 ** r_exp
    q = stored.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), stored), "the e4m3 form of the activation is not exact"
    return q.view(torch.uint8).contiguous(), torch.tensor([r_exp], dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _keep():
    """the kernels' keep decision for element (m, f) of an [.][512] tensor, from the numpy restatement of csrc/common.cuh
    dropout_quad: quad index (m * 512 + f) >> 2, draw f & 3"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dropout_hash_check as dh
    idx = np.arange(M_MAX, dtype=np.uint64)[:, None] * np.uint64(128) + np.arange(128, dtype=np.uint64)[None, :]
    a, b = dh.quad(idx, np.uint64(DP_KEY))
    draws = np.stack(dh.draws(a, b), axis=-1).reshape(M_MAX, 512)
    keep = torch.from_numpy(draws >= DP_THRESH).to(DEV)
    for M in sorted(set(FWD_M + WGRAD_M + DGRAD_M)):
        if M >= 31:
            n = M * 512
            share = float(keep[:M].sum()) / n
            assert abs(share - 0.5) <= 6 * (0.25 / n) ** 0.5, ("kept share", M, share)
    return keep


def _splits(M):
    """split_rows(M, kProjSplits, .): rows per split rounded up to 32, at least 32"""
    rps = max(32, -(-(-(-M // PROJ_SPLITS)) // 32) * 32)
    return -(-M // rps)


# ---- buffers -----------------------------------------------------------------------------------------------------------------------
def _buf(n, dtype=torch.float32, sentinel=SENTINEL32):
    """n elements and a guard behind them, all sentinel"""
    guard = GUARD_FLOATS
    t = torch.empty(n + guard, dtype=dtype, device=DEV)
    if dtype == torch.float32:
        t.view(torch.int32).fill_(sentinel)
    else:
        t.view(torch.int16).fill_(SENTINEL16)
    return t


def _untouched(tag, what, t, n, sentinel=SENTINEL32):
    tail = t[n:]
    if t.dtype == torch.float32:
        tail = tail.view(torch.int32)
        assert torch.equal(tail, torch.full_like(tail, sentinel)), (tag, "floats behind %s were written" % what)
    else:
        tail = tail.view(torch.int16)
        assert torch.equal(tail, torch.full_like(tail, SENTINEL16)), (tag, "elements behind %s were written" % what)


def _launch(kind, dtype, M, dropout=False, Wp=None, **bufs):
    from contrastiveprosthetics_amd import _lib
    o = _operands()
    d = _lib.cp_debug_proj_args()
    d.dtype, d.kind, d.M = (_lib.CP_F32 if dtype == F32 else _lib.CP_BF16), kind, M
    d.Wp = (o["Wp"] if Wp is None else Wp).data_ptr()
    d.scale, d.shift, d.coef = o["scale"].data_ptr(), o["shift"].data_ptr(), o["coef"].data_ptr()
    if kind != 0:
        d.dz = _typed("dz", dtype).data_ptr()
    for name, t in bufs.items():
        setattr(d, name, t.data_ptr() if t is not None else None)
    if d.act is None:
        d.act = _typed("R", dtype).data_ptr()
    if dropout:
        d.dp_thresh, d.dp_key, d.dp_inv_keep = DP_THRESH, DP_KEY, DP_INV_KEEP
    rows = ctypes.c_int32(-1)
    d.rows_out = ctypes.pointer(rows)
    _lib.check(_lib.load().cp_debug_proj(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "cp_debug_proj")
    torch.cuda.synchronize()
    return rows.value


def _act_args(r_exp):
    if r_exp is None:
        return {}
    act, word = _act8(r_exp)
    return dict(act=act, r_exp=word)


# ---- the preconditions of "tolerance zero", asserted on the reference ------------------------------------------------------
SEEN = {}


def _exact_values(tag, name, ref):
    """the values a kernel rounds to bf16 are bf16 numbers already"""
    assert torch.equal(ref, ref.bfloat16().double()), (tag, name)
    SEEN.setdefault(tag, {})["max |%s|" % name] = float(ref.abs().max())


def _exact_stat(tag, name, terms, step):
    """a column sum of `terms` is exact in float32 in any order and grouping: every term is an integer multiple of `step`, and even the
    column sums of |term| stay below 2^24 steps"""
    q = terms / step
    assert torch.equal(q, q.round()), (tag, name)
    top = float(q.abs().sum(0).max())
    assert top < 2 ** 24, (tag, name, top)
    SEEN.setdefault(tag, {})["sum |%s| / step" % name] = top


def _exact_acc(tag, name, a, b, step):
    """every accumulator of the product a^T-or-a times b is exact in float32 in any order: the operands are multiples of steps whose
    product is `step`, and sum |a| |b| stays below 2^24 steps"""
    q = (a.abs() @ b.abs()) / step
    assert torch.equal(q, q.round()), (tag, name)
    top = float(q.max())
    assert top < 2 ** 24, (tag, name, top)
    SEEN.setdefault(tag, {})["sum |%s| / step" % name] = top


def _report(tag):
    print("\n[proj_exact] %s: %s (2^24 = 16777216)" % (tag, ", ".join("%s %g" % kv for kv in SEEN.get(tag, {}).items())))


def _where(got, ref):
    bad = got != ref                                            # (a sentinel NaN left in place differs from everything)
    rows = bad.any(1).nonzero().flatten()
    cols = bad.any(0).nonzero().flatten()
    return "%d elements differ; rows %s .. %s (%d rows), 32-row tiles %s, columns %s .. %s (%d columns)" % (
        int(bad.sum()), rows[:8].tolist(), rows[-3:].tolist(), rows.numel(), torch.unique(rows // 32)[:12].tolist(),
        cols[:8].tolist(), cols[-3:].tolist(), cols.numel())


def _same(tag, what, got, ref):
    got, ref = got.double(), ref.double()
    if got.dim() == 1:
        got, ref = got[None], ref[None]
    assert torch.equal(got, ref), (tag, what, _where(got, ref))


# ---- references (float64) ----------------------------------------------------------------------------------------------------------
def _f64(M, Wp=None):
    o = _operands()
    return dict(d=o["dz"][:M, :16].double(), r=o["R"][:M].double(), s=o["scale"].double(), t=o["shift"].double(),
                W=(o["Wp"] if Wp is None else Wp).double(), keep=_keep()[:M])


def _dropped_activation(tag, v):
    """u = dropout(s r + t) as bn_drop_chunk forms and rounds it"""
    u = torch.where(v["keep"], (v["s"] * v["r"] + v["t"]) * DP_INV_KEEP, torch.zeros_like(v["r"]))
    _exact_values(tag, "u", u)
    return u


def ref_forward(tag, M, dropout):
    v = _f64(M)
    if dropout:
        a, w, b = _dropped_activation(tag, v), v["W"], torch.zeros(16, dtype=torch.float64, device=DEV)
    else:
        a, w, b = v["r"], v["W"] * v["s"], v["W"] @ v["t"]
        _exact_values(tag, "Wp s", w)
        _exact_acc(tag, "Wp t", v["W"], v["t"][:, None], 1.0)
    _exact_acc(tag, "a w", a, w.T, 0.5)
    return dict(w=w, b=b, z=a @ w.T + b)


def ref_wgrad_plain(tag, M, Wp=None, step=1.0):
    v = _f64(M, Wp)
    dzsum = v["d"].sum(0)
    P = v["d"].T @ v["r"]
    _exact_stat(tag, "dz", v["d"], 1.0)
    _exact_acc(tag, "dz r", v["d"].T, v["r"], 1.0)
    dW = v["s"] * P + v["t"] * dzsum[:, None]
    s1, s2 = (v["W"] * dzsum[:, None]).sum(0), (v["W"] * P).sum(0)
    _exact_stat(tag, "Wp dzsum", v["W"] * dzsum[:, None], step)
    _exact_stat(tag, "Wp P", v["W"] * P, step)
    assert torch.equal(s1, s1.float().double()) and torch.equal(s2, s2.float().double()), tag
    return dict(dzsum=dzsum, P=P, dW=dW, row=torch.cat([s1, s2]))


def ref_wgrad_drop(tag, M, r_exp=None, Wp=None):
    """both routes behind the dropout: dW = dz^T u (two products) = (s A + t B) / (1 - p) (one pass), and the finish kernel's rows"""
    v = _f64(M, Wp)
    u = _dropped_activation(tag, v)
    k = v["keep"].double()
    dW = v["d"].T @ u
    _exact_acc(tag, "dz u", v["d"].T, u, 1.0)
    e = 0 if r_exp is None else r_exp
    A, B = v["d"].T @ (k * v["r"] * 2.0 ** e), v["d"].T @ k                   # A in stored units, as the slabs hold it
    _exact_acc(tag, "dz keep r", v["d"].T, k * v["r"] * 2.0 ** e, 0.5)
    A1, B1 = A * DP_INV_KEEP * 2.0 ** -e, B * DP_INV_KEEP
    assert torch.equal(v["s"] * A1 + v["t"] * B1, dW), (tag, "the two routes' references differ")
    w = v["W"].bfloat16().double()                                            # the finish kernel rounds Wp to bf16
    rows = torch.stack([torch.stack([(w * B1)[4 * y:4 * y + 4].sum(0), (w * A1)[4 * y:4 * y + 4].sum(0)]) for y in range(PROJ_FINISH_ROWS)])
    g = k * (v["d"] @ w) * DP_INV_KEEP                                        # the masked gradient into fc7's BatchNorm
    _exact_stat(tag, "g", g, 1.0)
    _exact_stat(tag, "g r", g * v["r"], 1.0)
    assert torch.equal(rows[:, 0].sum(0), g.sum(0)) and torch.equal(rows[:, 1].sum(0), (g * v["r"]).sum(0)), (tag, "rows against sum g, sum g r")
    assert torch.equal(rows, rows.float().double()), tag
    return dict(dW=dW, AB=torch.cat([A, B]), rows=rows, g_sum=g.sum(0), gr_sum=(g * v["r"]).sum(0))


def ref_dgrad(tag, M, Wp=None):
    v = _f64(M, Wp)
    ca, cb, cz = (c.double() for c in _operands()["coef"])
    w = v["W"].bfloat16().double()                                            # transpose_w_kernel<bf16> rounds Wp
    acc = v["d"] @ w
    _exact_acc(tag, "dz Wp", v["d"], w, 1.0)
    g = torch.where(v["keep"], acc * DP_INV_KEEP, torch.zeros_like(acc))
    _exact_values(tag, "g", g)
    C = torch.where(v["r"] > 0, ca * g + cb * v["r"] + cz, torch.zeros_like(g))
    _exact_values(tag, "C", C)
    _exact_stat(tag, "C", C, 0.5)
    return dict(wt=w.T, acc=acc, C=C, dropped=cb * v["r"] + cz)


# ---- kind 0 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", FWD_M)
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("dtype,r_exp", TYPES, ids=TYPE_IDS)
def test_forward_is_exact(dtype, r_exp, dropout, M):
    tag = "forward %s %s %s M=%d" % (_id_dtype(dtype), _id_exp(r_exp), "p=0.5" if dropout else "no dropout", M)
    ref = ref_forward(tag, M, dropout)
    T = torch.float32 if dtype == F32 else torch.bfloat16
    w32, blast, z = _buf(32 * 512, T), _buf(16), _buf(M * 16, sentinel=SENTINEL_Z)                  # (the guard behind z: 512 rows of 16)
    rows = _launch(0, dtype, M, dropout=dropout, w32=w32, blast=blast, out=z, **_act_args(r_exp))
    assert rows == 0, (tag, rows)
    wl = w32[:32 * 512].view(32, 512)
    _same(tag, "wlast rows 0..15", wl[:16], ref["w"])
    assert not bool(wl[16:].double().abs().any()), (tag, "wlast rows 16..31 are not zero")
    _untouched(tag, "wlast", w32, 32 * 512)
    _same(tag, "blast", blast[:16], ref["b"])
    _untouched(tag, "blast[16]", blast, 16)
    _same(tag, "z", z[:M * 16].view(M, 16), ref["z"])
    _untouched(tag, "z's row M - 1", z, M * 16, SENTINEL_Z)
    _report(tag)


# ---- kind 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", WGRAD_M + [16485])
@pytest.mark.parametrize("dtype,r_exp", TYPES, ids=TYPE_IDS)
def test_weight_gradient_without_dropout_is_exact(dtype, r_exp, M):
    tag = "wgrad %s %s M=%d" % (_id_dtype(dtype), _id_exp(r_exp), M)
    ref = ref_wgrad_plain(tag, M)
    _check_plain_wgrad(tag, dtype, r_exp, M, ref)
    _report(tag)


def _check_plain_wgrad(tag, dtype, r_exp, M, ref, Wp=None):
    S = _splits(M)
    slabs, dW, praw, dzsum, part = _buf(S * 64 * 512), _buf(16 * 512), _buf(16 * 512), _buf(16), _buf(2 * 512)
    rows = _launch(1, dtype, M, Wp=Wp, slabs=slabs, out=dW, praw=praw, dzsum=dzsum, partials=part, **_act_args(r_exp))
    assert rows == S, (tag, "splits", rows, S)
    _same(tag, "dzsum", dzsum[:16], ref["dzsum"])
    _untouched(tag, "dzsum", dzsum, 16)
    total = slabs[:S * 64 * 512].view(S, 64, 512).double().sum(0)
    _same(tag, "slabs summed, rows 0..15", total[:16], ref["P"])
    assert not bool(total[16:].abs().any()), (tag, "slab rows 16..63 are not zero")
    _untouched(tag, "the last slab", slabs, S * 64 * 512)
    _same(tag, "praw", praw[:16 * 512].view(16, 512), ref["P"])
    _untouched(tag, "praw", praw, 16 * 512)
    _same(tag, "dW", dW[:16 * 512].view(16, 512), ref["dW"])
    _untouched(tag, "dW", dW, 16 * 512)
    _same(tag, "the partial row [2][512]", part[:1024], ref["row"])
    _untouched(tag, "the partial row", part, 1024)                  # (dz's <= 64 rows of 16 column sums passed through the same 1,024 floats)


# ---- kind 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", WGRAD_M)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id_dtype)
def test_two_product_weight_gradient_behind_the_dropout_is_exact(dtype, M):
    tag = "wgrad two products %s M=%d" % (_id_dtype(dtype), M)
    ref = ref_wgrad_drop(tag, M)
    S = _splits(M)
    slabs, dW = _buf(S * 64 * 512), _buf(16 * 512)
    rows = _launch(2, dtype, M, dropout=True, slabs=slabs, out=dW)
    assert rows == S, (tag, "splits", rows, S)
    total = slabs[:S * 64 * 512].view(S, 64, 512).double().sum(0)
    _same(tag, "slabs summed, rows 0..15", total[:16], ref["dW"])
    assert not bool(total[16:].abs().any()), (tag, "slab rows 16..63 are not zero")
    _untouched(tag, "the last slab", slabs, S * 64 * 512)
    _same(tag, "dW", dW[:16 * 512].view(16, 512), ref["dW"])
    _untouched(tag, "dW", dW, 16 * 512)
    _report(tag)


# ---- kind 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", WGRAD_M)
@pytest.mark.parametrize("r_exp", R_EXPS, ids=_id_exp)
def test_one_pass_weight_gradient_behind_the_dropout_is_exact(r_exp, M):
    tag = "wgrad one pass %s M=%d" % (_id_exp(r_exp), M)
    ref = ref_wgrad_drop(tag, M, r_exp)
    _check_one_pass(tag, r_exp, M, ref)
    _report(tag)


def _check_one_pass(tag, r_exp, M, ref, Wp=None):
    S = _splits(M)
    slabs, dW, part = _buf(S * 32 * 512), _buf(16 * 512), _buf(PROJ_FINISH_ROWS * 2 * 512)
    rows = _launch(3, BF16, M, dropout=True, Wp=Wp, slabs=slabs, out=dW, partials=part, **_act_args(r_exp))
    assert rows == S, (tag, "splits", rows, S)
    total = slabs[:S * 32 * 512].view(S, 32, 512).double().sum(0)
    _same(tag, "slabs summed: A = dz^T (keep r), B = dz^T keep", total, ref["AB"])
    _untouched(tag, "the last slab", slabs, S * 32 * 512)
    _same(tag, "dW", dW[:16 * 512].view(16, 512), ref["dW"])
    _untouched(tag, "dW", dW, 16 * 512)
    got = part[:PROJ_FINISH_ROWS * 1024].view(PROJ_FINISH_ROWS, 2, 512).double()
    _same(tag, "rows summed: sum g", got[:, 0].sum(0), ref["g_sum"])
    _same(tag, "rows summed: sum g r", got[:, 1].sum(0), ref["gr_sum"])
    _same(tag, "rows[4][2][512]", got.view(-1, 512), ref["rows"].view(-1, 512))
    _untouched(tag, "the fourth row", part, PROJ_FINISH_ROWS * 1024)


# ---- kind 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", DGRAD_M)
def test_data_gradient_behind_the_dropout_is_exact(M):
    tag = "dgrad M=%d" % M
    ref = ref_dgrad(tag, M)
    C = _check_dgrad(tag, M, ref)
    # what the outputs show of the mask without knowing the hash: where the product and the activation are live, an element is either
    # the dropped value cb r + cz or not, and about half are kept
    v = _f64(M)
    live = (v["r"] > 0) & (ref["acc"] != 0)
    count = int(live.sum())
    share = float(((C != ref["dropped"]) & live).sum()) / count
    assert abs(share - 0.5) <= 6 * (0.25 / count) ** 0.5, (tag, share, count)
    _report(tag)


def _check_dgrad(tag, M, ref, Wp=None):
    n_rows = min(-(-M // PROJ_RT), PROJ_WORKERS)
    w32, part = _buf(512 * 64, torch.bfloat16), _buf(n_rows * 512)
    C = torch.empty(M + GUARD_ROWS, 512, dtype=torch.bfloat16, device=DEV)
    C.view(torch.int16).fill_(SENTINEL16)
    rows = _launch(4, BF16, M, dropout=True, Wp=Wp, w32=w32, out=C, partials=part)
    assert rows == n_rows, (tag, "partial rows", rows, n_rows)
    wt = w32[:512 * 64].view(512, 64)
    _same(tag, "wlast_t columns 0..15", wt[:, :16], ref["wt"])
    assert not bool(wt[:, 16:].double().abs().any()), (tag, "wlast_t columns 16..63 are not zero")
    _untouched(tag, "wlast_t", w32, 512 * 64)
    _same(tag, "C", C[:M], ref["C"])
    guard = C[M:].view(torch.int16)
    assert torch.equal(guard, torch.full_like(guard, SENTINEL16)), (tag, "rows behind M were written")
    _same(tag, "partial rows summed", part[:n_rows * 512].view(n_rows, 512).double().sum(0), ref["C"].sum(0))
    _untouched(tag, "the last partial row", part, n_rows * 512)
    return C[:M].double()


# ---- where each kernel rounds the weight ---------------------------------------------------------------------------------------------
def test_where_the_weight_is_rounded():
    """One entry of Wp is 1 + 2^-10: a float32 that bf16 rounds to 1.  What the code does today, pinned (the bounds of
    tests/test_gpu_fullsize.py rest on it): proj_wgrad_finish_kernel's rows and the data gradient (transpose_w_kernel<bf16>) use
    round_bf16(Wp), so both see 1; bn_bwd_sums_from_wgrad_kernel multiplies by the float32 value, so its sums carry the 2^-10.
    The entry sits where dzsum, the raw product and both one-pass products are non-zero (asserted), so each reference differs from
    the one the other rounding would give; the sums stay multiples of 2^-10 far below 2^24 of them."""
    M = 64
    o = _operands()
    plain0, drop0 = ref_wgrad_plain("rounding", M), ref_wgrad_drop("rounding", M)
    AB = drop0["AB"]
    ok = (plain0["P"] != 0) & (plain0["dzsum"][:, None] != 0) & (AB[:16] != 0) & (AB[16:] != 0) & (o["Wp"] != 0)
    assert bool(ok.any()), "no entry of Wp shows in every sum at this M"
    j, f = (int(x) for x in ok.nonzero()[0])
    Wp = o["Wp"].clone()
    Wp[j, f] *= 1.0 + 2.0 ** -10
    assert float(Wp[j, f]) != float(Wp[j, f].bfloat16()) and float(Wp[j, f].bfloat16()) == float(o["Wp"][j, f])
    Wp = Wp.contiguous()
    tag = "rounding Wp[%d][%d] = %r M=%d" % (j, f, float(Wp[j, f]), M)
    # the float32 value: bn_bwd_sums_from_wgrad_kernel
    plain = ref_wgrad_plain(tag, M, Wp, step=2.0 ** -10)
    assert not torch.equal(plain["row"], plain0["row"]), "the case does not tell the two roundings apart"
    _check_plain_wgrad(tag, BF16, None, M, plain, Wp=Wp)
    # the rounded value: proj_wgrad_finish_kernel's rows and proj_dgrad_kernel's operand equal those of the unchanged weight
    drop = ref_wgrad_drop(tag, M, None, Wp)
    assert torch.equal(drop["rows"], drop0["rows"])
    _check_one_pass(tag, None, M, drop, Wp=Wp)
    dg = ref_dgrad(tag, M, Wp)
    assert torch.equal(dg["wt"], o["Wp"].double().T)
    _check_dgrad(tag, M, dg, Wp=Wp)
    _report(tag)
