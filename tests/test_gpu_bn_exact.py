"""The f32 / bf16 BatchNorm and weight-preparation launches that sit between the GEMMs of the large-batch step (csrc/kernels_misc.cuh),
on their own, one sequence at a time through cp_debug_bn, against float64 references at ragged row counts.

What runs (include/cpnative.h, cp_debug_bn; the launch functions, grids, caps and the pre-reduce rule are the step's own,
csrc/encoder_api.cuh):

    kind 0   PreReduce (reduce_rows_kernel past 2,048 partial rows) + bn_finalize_kernel -> stats[4][C], the running buffers
    kind 1   bn_running_stats_kernel -> nine tables;  the eight-job fold_linear_batch_kernel<T> -> eight images, eight biases
    kind 2   PreReduce + bn_bwd_finalize_kernel -> coef[3][C], dgamma, dbeta              (C, nfold) = (512, 1), (64, 1), (64, 12)
    kind 3   bn_dropout_apply_kernel<T> on grid_rows(M, rpp, CAP_BDA16) -> u[M][512]
    kind 4   bn_relu_bwd_kernel<T> in place + colsum_finalize_kernel -> g[M][C], partials[gb][C], db[C]       C = 512 | 64
    kind 5   fold_linear_kernel<T> (modes 0, 1), the four-job fold_copy_batch_kernel<T>, the eight-job transpose_w_batch_kernel<T>

The references are tests/bn_reference.py, which tests/test_bn_reference_host.py anchors to torch.nn.BatchNorm and autograd.

STREAMING KERNELS (kinds 3, 4): tolerance zero.  The recipe of tests/test_gpu_proj_exact.py: g ternary (-1 / 1 with probability 1/16
each), r = relu(randint(-2, 4)), scale and ca from {0.5, 1, 2}, shift, cb and cz small integers, dropout at p = 0.5 (threshold 32768,
1 / (1 - p) = 2).  Every output is a multiple of 0.5 well inside bf16 and every per-block column sum is exact in float32 in any order;
both are asserted on the float64 reference before anything is compared (`_exact_values`, `_exact_stat`), and each case prints the
largest value and sum it saw (pytest -s).  One planted column (5) of r is non-positive (0 and -1 alternating) under cz = 1000: the output
there must be exactly 0 and so must its column sum.  Compared with torch.equal: every element below M; each partial row against the
sum over that block's own rows (m = block * rpp + rr, stepping by grid * rpp); db against the float64 column sum; rows_out against
min(ceil(M / rpp), cap); the NaN-pattern sentinels behind row M, behind the last partial row, behind db and in the pre-reduce scratch.
The mask of kind 3 is held element by element to tools/dropout_hash_check.py at (key, m, 512, f) -- the restatement the GEMM-side tests
use, so producer and consumers of u are tied to one hash; its kept share lies within 6 binomial standard deviations of 0.5 at every
M >= 31 used here (tests/test_bn_reference_host.py checks that on the CPU for this key).

Row counts of kinds 3 and 4.  A block holds rpp = 256 / (C / EPC) rows per pass (EPC = 8 bf16 | 4 f32 elements per 16-byte chunk); the
grid is min(ceil(M / rpp), cap), so the cap is reached past cap * rpp rows and the row step is then cap * rpp.  The kernels walk
`for (; m + step < M; m += 2 step)` in pairs and finish with `if (m < M)`:
    C = 512 bf16 (rpp 4, cap 512: 2,048 rows)   1, 3, 4 (one full block), 5 (a second block with one row), 2,047, 2,048 (the last
                                                uncapped grid: tails only), 2,049 (capped: thread 0 of block 0 takes the first
                                                unrolled pair, nobody a tail behind it), 4,096 (pairs only, no tail), 4,097 (pair +
                                                tail), 6,145 (two pairs in one thread; others pair + tail), 8,193 (two pairs + tail)
    C = 512 f32  (rpp 2, cap 512: 1,024 rows)   the same at half: 1, 2, 3, 1,023, 1,024, 1,025, 2,048, 2,049, 3,073, 4,097
    C = 64  bf16 (rpp 32, cap 2,048: 65,536)    1, 31, 32, 33, 65,535, 65,536, 65,537 (first pair), 131,073 (pair + tail)
    C = 64  f32  (rpp 16, cap 2,048: 32,768)    1, 15, 16, 17, 32,767, 32,768, 32,769, 65,537
C = 64 at its cap is the only place where colsum_finalize_kernel sees exactly FIN_DIRECT_ROWS = 2,048 partial rows: no pre-reduce, four
batches of eight per lane and no tail.  (The list of the issue was re-derived from grid_rows and the two loops; no number moved.)

FINALIZE KERNELS (kinds 0, 2), two tiers, at the partial-row counts 1, 63, 64 (one row per lane), 65 (lane 0 a second row), 448, 449
(lane 0's first batch of eight: rows 0, 64, .., 448), 512, 513 (a batch and a tail), 2,048 (four batches per lane, no tail, no
pre-reduce), 2,049 (pre-reduce: 32 slices, slice 0 with 65 rows -- 17 in its first lane), 5,000 (slices of 156 and 157 rows: two
eight-deep batches of reduce_rows_kernel do not fit, one does); kind 2 also 4 (PROJ_FINISH_ROWS; 1 and CONV2_FINISH_ROWS = 64 are in
the list).
  * Exact tier.  The rows are small integers (multiples of a step where unscale_exp < 0) with sum |x| < 2^24 steps, so every float32
    or float64 sum has one right answer in any order, the float32 pre-reduce included.  count = 4,096; per column the mean p / 4, the
    unbiased variance an integer q and var = q (1 - 1 / count) are planted through the column totals, so that mean, E[x^2], var and
    var count / (count - 1) are float32 numbers and s2 / count - mean^2 is exact contracted or not (asserted in plant_forward_totals).
    mean, the running buffers (momentum 1/2, priors multiples of 1/8: new = (1 - m) old + m batch with the UNBIASED variance) and, in
    kind 2, every output (mean a multiple of 1/4, invstd a power of two, scale = 1.5 invstd | 3 invstd | 0.5 invstd: no float64
    operation rounds, so coef is the single float32 rounding of the exact value) are compared with torch.equal.  Planted, kind 0:
    column 1 has s2 / count = mean^2 - 1 (the clamp: var 0, invstd = 1 / sqrt(eps)); count = 1; update_running = 0 (buffers
    bit-identical); no running buffers; unscale_exp in {0, 3, -2}; C = 64 (four blocks of 16 columns, every column its own values).
    Kind 2: nfold = 12 with every fold its own values; `local`; gamma-scale != 1; channel 2 with sum g = sum g r = 0.
  * Real-valued tier.  Partial rows are float32 sums of 8 normally distributed activations (8 float32 additions each), |mean| / std
    100 in columns 0..7 and around 1 elsewhere.  The reference is fed the same float32 rows: the rows themselves, or past 2,048 of
    them the 32 rows of the pre-reduce restated in float32 in reduce_rows_kernel's own order (bn_reference.reduce_rows_f32), which the
    scratch must equal bit for bit and which is itself held to the float64 slice sums within depth * 2^-24 * sum |x|.  The bounds
    are derived in bn_reference.stats_bounds / coef_bounds / running_stats_bounds, not observed: the chain mean = (float) mu;
    var = (float) vb; x = var + eps; invstd = 1.0f / sqrtf(x); scale = gamma * invstd; shift = beta - mean * scale, each correctly
    rounded operation charged 0.5 ulp (2^-24 relative), sqrtf and the division 1 ulp each -- no figure for either was found in the
    ROCm headers or documents next to the compiler, so the fallback the issue names is taken -- which makes invstd (1 + 2 + 2) 2^-24
    relative, scale one more, shift the absolute bound that follows from |mean scale|; coef, dgamma and dbeta the single rounding of a
    float64 expression whose own error is bounded with sums of magnitudes.  Each case prints its worst error / bound ratio.

WEIGHT PREPARATION (kind 5, and kind 1's folds).  W ternary (coded in the mode-1 cases: W[j][c * 12 + w] = (-1)^j (1 + c + 64 w), for
bf16 1 + c % 16 + 16 w, so a swapped k / 12 and k % 12 cannot cancel), s from {0.25 .. 4}, t a multiple of 1/4: the folded weight and
the bias b + W t have one right answer.  Every element of every image is compared with torch.equal against the float64 statement of
the layout (rounded by .bfloat16() for bf16), the padding as zeros (rows 16..31 of the projection image, columns 16..63 of its
transpose), the sentinel behind every image and bias.

The inputs hold live data behind row M, so a load that lost its row guard shows in the sums."""
import ctypes
import functools
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as br  # noqa: E402  (tests/bn_reference.py)

pytestmark = pytest.mark.gpu

DEV = "cuda" if torch.cuda.is_available() else "cpu"
F32, BF16 = 0, 1
GUARD_ROWS = 64
GUARD_FLOATS = 8192
SENTINEL16 = 0x7FA5                     # a bf16 NaN
SENTINEL32 = 0x7FC0BEEF                 # a float32 NaN
PLANT = 5                               # the column of r that is never positive
CAP512, CAP64 = 512, 2048               # CAP_BDA16 = CAP_BRB16, and conv2's BatchNorm (csrc/encoder_api.cuh)
EPS = 1e-5

M512 = {BF16: [1, 3, 4, 5, 2047, 2048, 2049, 4096, 4097, 6145, 8193], F32: [1, 2, 3, 1023, 1024, 1025, 2048, 2049, 3073, 4097]}
M64 = {BF16: [1, 31, 32, 33, 65535, 65536, 65537, 131073], F32: [1, 15, 16, 17, 32767, 32768, 32769, 65537]}
STREAM512 = [(d, m) for d in (BF16, F32) for m in M512[d]]
STREAM64 = [(d, m) for d in (BF16, F32) for m in M64[d]]
FIN_ROWS = [1, 63, 64, 65, 448, 449, 512, 513, 2048, 2049, 5000]
SHAPES = [(512, 1), (64, 1), (64, 12)]
_id_dtype = lambda d: "f32" if d == F32 else "bf16"
_id_stream = lambda p: "%s-M%d" % (_id_dtype(p[0]), p[1])
_torch_t = lambda d: torch.float32 if d == F32 else torch.bfloat16
_rpp = lambda C, d: 256 // (C // (4 if d == F32 else 8))


# ---- buffers, launches ------------------------------------------------------------------------------------------------------------
def _buf(n, dtype=torch.float32):
    """n elements and a guard behind them, all sentinel"""
    t = torch.empty(n + GUARD_FLOATS, dtype=dtype, device=DEV)
    if dtype == torch.float32:
        t.view(torch.int32).fill_(SENTINEL32)
    else:
        t.view(torch.int16).fill_(SENTINEL16)
    return t


def _filled(values):
    """a sentinel buffer whose first elements are `values`"""
    t = _buf(values.numel(), values.dtype)
    t[:values.numel()] = values.reshape(-1)
    return t


def _untouched(tag, what, t, n):
    tail = t[n:]
    tail = tail.view(torch.int32) if t.dtype == torch.float32 else tail.view(torch.int16)
    want = SENTINEL32 if t.dtype == torch.float32 else SENTINEL16
    assert torch.equal(tail, torch.full_like(tail, want)), (tag, "elements behind %s were written" % what)


def _launch(kind, dtype=F32, **fields):
    from contrastiveprosthetics_amd import _lib
    d = _lib.cp_debug_bn_args()
    d.dtype, d.kind = (_lib.CP_F32 if dtype == F32 else _lib.CP_BF16), kind
    keep = []
    for name, v in fields.items():
        if isinstance(v, torch.Tensor):
            setattr(d, name, v.data_ptr())
        elif isinstance(v, (list, tuple)):
            arr = getattr(d, name)
            for i, t in enumerate(v):
                arr[i] = t.data_ptr() if t is not None else None
        elif isinstance(v, ctypes.Structure):
            keep.append(v)
            setattr(d, name, ctypes.addressof(v))
        elif v is not None:
            setattr(d, name, v)
    rows = ctypes.c_int32(-1)
    d.rows_out = ctypes.pointer(rows)
    _lib.check(_lib.load().cp_debug_bn(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "cp_debug_bn")
    torch.cuda.synchronize()
    return rows.value


# ---- the preconditions of "tolerance zero", asserted on the reference ------------------------------------------------------------
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


def _report(tag):
    print("\n[bn_exact] %s: %s" % (tag, ", ".join("%s %g" % kv for kv in SEEN.get(tag, {}).items())))


def _where(got, ref):
    bad = got != ref                                            # (a sentinel NaN left in place differs from everything)
    rows = bad.any(1).nonzero().flatten()
    cols = bad.any(0).nonzero().flatten()
    return "%d elements differ; rows %s .. %s (%d rows), columns %s .. %s (%d columns)" % (
        int(bad.sum()), rows[:8].tolist(), rows[-3:].tolist(), rows.numel(), cols[:8].tolist(), cols[-3:].tolist(), cols.numel())


def _same(tag, what, got, ref):
    got, ref = got.double(), ref.double()
    if got.dim() == 1:
        got, ref = got[None], ref[None]
    assert torch.equal(got, ref), (tag, what, _where(got, ref))


def _within(tag, what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())      # (a bound of 0: equality)
    worst = float(ratio.max())
    SEEN.setdefault(tag, {})["%s err / bound" % what] = worst
    assert worst <= 1.0, (tag, what, "worst error / bound", worst, "at", int(ratio.reshape(-1).argmax()),
                          "error", float(err.reshape(-1)[ratio.reshape(-1).argmax()]))


# ---- operands of the streaming kernels -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream_operands(C):
    """the recipe of the module docstring, made once per width: slices [:M] serve every case"""
    gen = torch.Generator(device=DEV).manual_seed(7300 + C)
    rows = max(M512[BF16] if C == 512 else M64[BF16]) + GUARD_ROWS
    g = br.ternary((rows, C), gen, 16, DEV)
    r = torch.relu(torch.randint(-2, 4, (rows, C), generator=gen, device=DEV).float())
    r[:, PLANT] = -(torch.arange(rows, device=DEV) % 2).float()
    pick = torch.tensor([0.5, 1.0, 2.0], device=DEV)
    stats = torch.zeros(4, C, device=DEV)
    stats[2] = pick[torch.randint(0, 3, (C,), generator=gen, device=DEV)]
    stats[3] = torch.randint(-2, 3, (C,), generator=gen, device=DEV).float()
    ca = pick[torch.randint(0, 3, (C,), generator=gen, device=DEV)]
    cb = torch.randint(-1, 2, (C,), generator=gen, device=DEV).float()
    cz = torch.randint(-2, 3, (C,), generator=gen, device=DEV).float()
    cz[PLANT] = 1000.0
    return dict(g=g, r=r, stats=stats.contiguous(), coef=torch.stack([ca, cb, cz]).contiguous())


@functools.lru_cache(maxsize=None)
def _typed(C, name, dtype):
    """g or r as the kernels read it (the values are bf16 numbers: the conversion is exact)"""
    return _stream_operands(C)[name].to(_torch_t(dtype)).contiguous()


@functools.lru_cache(maxsize=None)
def _keep():
    counts = sorted(set(M512[BF16] + M512[F32]))
    keep = br.keep_mask(br.DP_KEY, max(counts), br.DP_THRESH)
    for M in counts:
        if M >= 31:
            ok, share = br.kept_share_ok(keep, M)
            assert ok, ("kept share", M, share)
    return torch.from_numpy(keep).to(DEV)


# ---- kind 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,M", STREAM512, ids=[_id_stream(p) for p in STREAM512])
def test_dropout_apply_is_exact(dtype, M):
    """bn_dropout_apply_kernel<T>: 1..2,048 (f32 1,024) rows one tail per thread, then the capped grid's pairs and tails (docstring)"""
    tag = "dropout apply %s M=%d" % (_id_dtype(dtype), M)
    o = _stream_operands(512)
    ref = br.ref_dropout_apply(o["r"][:M], o["stats"][2], o["stats"][3], _keep()[:M], br.DP_INV_KEEP)
    _exact_values(tag, "u", ref)
    u = torch.empty(M + GUARD_ROWS, 512, dtype=_torch_t(dtype), device=DEV)
    u.view(torch.int32 if dtype == F32 else torch.int16).fill_(SENTINEL32 if dtype == F32 else SENTINEL16)
    rows = _launch(3, dtype, M=M, r=_typed(512, "r", dtype), stats=o["stats"], g=u, dp_thresh=br.DP_THRESH, dp_key=br.DP_KEY,
                   dp_inv_keep=br.DP_INV_KEEP)
    assert rows == 0, (tag, rows)
    _same(tag, "u", u[:M], ref)
    _untouched(tag, "row M - 1 of u", u.view(-1), M * 512)
    if M >= 31:      # what the output shows of the mask without knowing the hash: where s r + t is live, about half is kept
        live = (o["stats"][2].double() * o["r"][:M].double() + o["stats"][3].double()) != 0
        n = int(live.sum())
        share = float(((u[:M].double() != 0) & live).sum()) / n
        assert abs(share - 0.5) <= 6 * (0.25 / n) ** 0.5, (tag, share, n)
    _report(tag)


# ---- kind 4 ---------------------------------------------------------------------------------------------------------------------------
def _check_relu_bwd(tag, C, dtype, M):
    o = _stream_operands(C)
    rpp, cap = _rpp(C, dtype), (CAP512 if C == 512 else CAP64)
    gb = min(-(-M // rpp), cap)
    ref = br.ref_bn_relu_bwd(o["g"][:M], o["r"][:M], o["coef"])
    _exact_values(tag, "g_y", ref)
    _exact_stat(tag, "g_y", ref, 0.5)
    assert not bool(ref[:, PLANT].any()), (tag, "the planted column's reference is not zero")
    blk = (torch.arange(M, device=DEV) // rpp) % gb                      # block of row m = block * rpp + rr + k * grid * rpp
    part_ref = torch.zeros(gb, C, dtype=torch.float64, device=DEV).index_add_(0, blk, ref)
    T = _torch_t(dtype)
    g = torch.empty(M + GUARD_ROWS, C, dtype=T, device=DEV)
    g.view(torch.int32 if dtype == F32 else torch.int16).fill_(SENTINEL32 if dtype == F32 else SENTINEL16)
    g[:M] = _typed(C, "g", dtype)[:M]
    part, db, scratch = _buf(gb * C), _buf(C), _buf(0)
    rows = _launch(4, dtype, M=M, C=C, g=g, r=_typed(C, "r", dtype), coef=o["coef"], partials=part, db=db, scratch=scratch)
    assert rows == gb, (tag, "partial rows", rows, gb)
    _same(tag, "g_y", g[:M], ref)
    _untouched(tag, "row M - 1 of g", g.view(-1), M * C)
    _same(tag, "partial rows", part[:gb * C].view(gb, C), part_ref)
    _untouched(tag, "the last partial row", part, gb * C)
    _same(tag, "db", db[:C], ref.sum(0))
    _untouched(tag, "db", db, C)
    _untouched(tag, "the pre-reduce scratch (at most 2,048 partial rows: no pre-reduce)", scratch, 0)
    assert not bool(g[:M, PLANT].double().any()) and float(db[PLANT]) == 0.0, (tag, "the planted column")
    _report(tag)


@pytest.mark.parametrize("dtype,M", STREAM512, ids=[_id_stream(p) for p in STREAM512])
def test_bn_relu_backward_is_exact_at_512_channels(dtype, M):
    """bn_relu_bwd_kernel<T> at C = 512 under CAP_BRB16, in place, + the bias gradient from its partial rows"""
    _check_relu_bwd("relu bwd C=512 %s M=%d" % (_id_dtype(dtype), M), 512, dtype, M)


@pytest.mark.parametrize("dtype,M", STREAM64, ids=[_id_stream(p) for p in STREAM64])
def test_bn_relu_backward_is_exact_at_64_channels(dtype, M):
    """the same at C = 64 under the cap 2,048 (conv2's BatchNorm): at the cap colsum_finalize_kernel folds exactly 2,048 rows"""
    _check_relu_bwd("relu bwd C=64 %s M=%d" % (_id_dtype(dtype), M), 64, dtype, M)


# ---- kind 0 ---------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _with_live_rows(rows, gen):
    """the partial rows as the kernel's input buffer: 8 rows of live data behind the last one"""
    n = rows.shape[0]
    extra = torch.randint(-500, 501, (8,) + tuple(rows.shape[1:]), generator=gen, device=DEV).float()
    return torch.cat([rows, extra]).contiguous(), n


def _affine(C, gen):
    pick = torch.tensor([0.5, 1.5, 3.0], device=DEV)
    return pick[torch.randint(0, 3, (C,), generator=gen, device=DEV)], torch.randint(-2, 3, (C,), generator=gen, device=DEV).float()


def _check_scratch(tag, rows, scratch, exact):
    """no pre-reduce up to 2,048 rows: the scratch keeps its sentinels; past them it holds the 32 float32 rows of the restatement, which
    is itself within its derived bound of the float64 slice sums.  Returns the rows the finalize kernel is handed."""
    n, width = rows.shape[0], rows[0].numel()
    if n <= br.FIN_DIRECT_ROWS:
        _untouched(tag, "the pre-reduce scratch (no pre-reduce)", scratch, 0)
        return rows
    fed = br.rows_as_finalized(rows)
    slices, bound = br.reduce_rows_bound(rows.reshape(n, -1))
    if exact:
        assert torch.equal(fed.reshape(32, -1).double(), slices), (tag, "the exact tier's pre-reduce is not exact")
    else:
        _within(tag, "pre-reduce restatement", fed.reshape(32, -1), slices, bound)
    _same(tag, "the pre-reduce scratch", scratch[:32 * width].view(32, width), fed.reshape(32, width))
    _untouched(tag, "the pre-reduce scratch", scratch, 32 * width)
    return fed


def _run_stats(tag, C, rows, count, gamma, beta, exact, unscale_exp=None, running=True, update=1, momentum=0.5, planted=None, tell_apart=True):
    gen = _gen("run", C, rows.shape[0])
    inp, n = _with_live_rows(rows, gen)
    stats, scratch = _buf(4 * C), _buf(32 * 2 * C)
    old_m = torch.randint(-16, 17, (C,), generator=gen, device=DEV).float() / 8
    old_v = torch.randint(0, 17, (C,), generator=gen, device=DEV).float() / 8
    rm, rv = (_filled(old_m), _filled(old_v)) if running else (None, None)
    exp_word = None if unscale_exp is None else torch.tensor([unscale_exp, 0, 0, 0], dtype=torch.int32, device=DEV)
    _launch(0, F32, M=n, C=C, count=float(count), rows=inp, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, update_running=update,
            momentum=momentum, eps=EPS, unscale_exp=exp_word, scratch=scratch, stats=stats)
    fed = _check_scratch(tag, rows, scratch, exact)
    e = unscale_exp or 0
    ref = br.ref_bn_stats(fed, count, gamma, beta, EPS, unscale_exp=e)
    bounds = br.stats_bounds(fed, count, ref, gamma, beta, EPS, unscale_exp=e)
    got = stats[:4 * C].view(4, C)
    _untouched(tag, "stats", stats, 4 * C)
    if exact:
        assert torch.equal(ref["mean"], planted["mean"]) and torch.equal(ref["var"], planted["var"]), (tag, "the reference misses what was planted")
        _same(tag, "mean", got[0], ref["mean"])
    else:
        _within(tag, "mean", got[0], ref["mean"], bounds["mean"])
    for i, name in ((1, "invstd"), (2, "scale"), (3, "shift")):
        _within(tag, name, got[i], ref[name], bounds[name])
    if running:
        _untouched(tag, "running_mean", rm, C)
        _untouched(tag, "running_var", rv, C)
        if not update:
            assert torch.equal(rm[:C], old_m) and torch.equal(rv[:C], old_v), (tag, "update_running = 0 changed the running buffers")
        elif exact:
            new_m, new_v = br.ref_running(old_m, ref["mean"], momentum), br.ref_running(old_v, ref["unbiased"], momentum)
            assert torch.equal(new_m, new_m.float().double()) and torch.equal(new_v, new_v.float().double()), (tag, "the running update is not exact")
            _same(tag, "running_mean", rm[:C], new_m)
            _same(tag, "running_var (the unbiased variance enters)", rv[:C], new_v)
            if tell_apart:
                assert not torch.equal(new_v, br.ref_running(old_v, ref["var"], momentum)), (tag, "biased and unbiased variance give the same update")
    return got, ref


def _exact_rows(C, n, count, gen, e=0, small=False, step=1.0):
    t = br.plant_forward_totals(C, count, gen, DEV, unscale_exp=e, small=small)
    return br.spread_totals(torch.cat([t["s1"], t["s2"]]), n, gen, step=step).reshape(n, 2, C), t


@pytest.mark.parametrize("n", FIN_ROWS)
@pytest.mark.parametrize("C", [64, 512])
def test_statistics_exact_tier(C, n):
    """bn_finalize_kernel on integer rows with planted totals: mean and the running buffers bit for bit, the clamp in column 1"""
    tag = "stats exact C=%d rows=%d" % (C, n)
    gen = _gen("stats exact", C, n)
    rows, t = _exact_rows(C, n, 4096, gen)
    gamma, beta = _affine(C, gen)
    got, ref = _run_stats(tag, C, rows, 4096, gamma, beta, True, planted=t)
    assert float(ref["var"][1]) == 0.0, tag                                    # the clamp: invstd = 1 / sqrt(eps) within the chain's bound
    _report(tag)


@pytest.mark.parametrize("case", ["count1", "no_update", "no_running", "exp0", "exp3", "exp-2"])
@pytest.mark.parametrize("n", [65, 2049])
@pytest.mark.parametrize("C", [64, 512])
def test_statistics_planted_edges(C, n, case):
    """count = 1 (the unbiased variance is the biased one), update_running = 0, no running buffers, unscale_exp in {0, 3, -2}"""
    tag = "stats %s C=%d rows=%d" % (case, C, n)
    gen = _gen("stats edges", C, n, case)
    count = 1 if case == "count1" else 4096
    e = {"exp0": 0, "exp3": 3, "exp-2": -2}.get(case)
    small = case in ("count1", "exp3", "exp-2")
    rows, t = _exact_rows(C, n, count, gen, e=e or 0, small=small, step=2.0 ** -8 if case in ("count1", "exp-2") else 1.0)
    gamma, beta = _affine(C, gen)
    if case == "count1":      # (biased = unbiased: the running update is compared all the same, the check that tells the two apart does not apply)
        assert torch.equal(t["unbiased"], t["var"]), tag
    _run_stats(tag, C, rows, count, gamma, beta, True, unscale_exp=e, running=case != "no_running", update=0 if case in ("no_update", "no_running") else 1,
               planted=t, tell_apart=case != "count1")
    _report(tag)


def _real_rows(C, n, gen, second=None):
    """n partial rows of 8 activations each: float32 sums of x and x^2, x ~ N(mu, sigma) per column, |mu| / sigma = 100 in columns 0..7"""
    sigma = torch.rand(C, generator=gen, device=DEV) * 1.5 + 0.5
    mu = torch.randn(C, generator=gen, device=DEV) * sigma
    mu[:8] = 100 * sigma[:8] * torch.tensor([1, -1, 1, -1, 1, -1, 1, -1], device=DEV)
    x = torch.randn(n, 8, C, generator=gen, device=DEV) * sigma + mu
    return torch.stack([x.sum(1), (x * x).sum(1)], 1).contiguous()           # float32 [n][2][C]


@pytest.mark.parametrize("n", FIN_ROWS)
@pytest.mark.parametrize("C", [64, 512])
def test_statistics_real_valued_tier(C, n):
    """bn_finalize_kernel on float32 sums of normal activations against float64 fed the same rows, within the derived float32 bounds"""
    tag = "stats real C=%d rows=%d" % (C, n)
    gen = _gen("stats real", C, n)
    rows = _real_rows(C, n, gen)
    gamma = torch.rand(C, generator=gen, device=DEV) + 0.5
    beta = torch.randn(C, generator=gen, device=DEV)
    _run_stats(tag, C, rows, 8 * n, gamma, beta, False, momentum=0.1)
    _report(tag)


# ---- kind 2 ---------------------------------------------------------------------------------------------------------------------------
def _run_coef(tag, C, nfold, rows, count, stats, exact, local=None):
    gen = _gen("coef", C, nfold, rows.shape[0])
    inp, n = _with_live_rows(rows, gen)
    W = C * nfold
    coef, dgamma, dbeta, scratch = _buf(3 * C), _buf(C), _buf(C), _buf(32 * 2 * W)
    _launch(2, F32, M=n, C=C, nfold=nfold, count=float(count), rows=inp, stats=stats, local=local, scratch=scratch, coef=coef, dgamma=dgamma,
            dbeta=dbeta)
    fed = _check_scratch(tag, rows, scratch, exact)
    ref = br.ref_bn_bwd_coef(fed, count, stats[0], stats[1], stats[2], C, nfold, local=local)
    for name, buf, k in (("coef", coef, 3 * C), ("dgamma", dgamma, C), ("dbeta", dbeta, C)):
        _untouched(tag, name, buf, k)
    got = dict(coef=coef[:3 * C].view(3, C), dgamma=dgamma[:C], dbeta=dbeta[:C])
    if exact:
        # no float64 operation of the expression rounds (docstring): another grouping of the same terms gives the same numbers
        m, i, s = stats[0].double(), stats[1].double(), stats[2].double()
        c1, c2 = ref["s1"] / count, (ref["s2"] * i - m * i * ref["s1"]) / count
        assert torch.equal(ref["coef"][2], s * m * i * c2 - s * c1) and torch.equal(ref["coef"][1], -(s * i) * c2), (tag, "the reference rounds in float64")
        for name in ("coef", "dgamma", "dbeta"):
            _same(tag, name, got[name], ref[name].float())
        assert torch.equal(ref["dbeta"], ref["dbeta"].float().double()), (tag, "dbeta is not a float32 number")
    else:
        bounds = br.coef_bounds(fed, count, stats[0], stats[1], stats[2], C, nfold, ref, local=local)
        _same(tag, "coef[0] = scale", got["coef"][0], stats[2])
        for name in ("coef", "dgamma", "dbeta"):
            _within(tag, name, got[name], ref[name], bounds[name])
    return got, ref


def _exact_bwd_stats(C, gen):
    stats = torch.zeros(4, C, device=DEV)
    stats[0] = torch.randint(-8, 9, (C,), generator=gen, device=DEV).float() / 4
    stats[1] = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (C,), generator=gen, device=DEV)]
    stats[2] = stats[1] * torch.tensor([0.5, 1.5, 3.0], device=DEV)[torch.randint(0, 3, (C,), generator=gen, device=DEV)]      # gamma-scale != 1
    return stats.contiguous()


@pytest.mark.parametrize("use_local", [False, True], ids=["plain", "local"])
@pytest.mark.parametrize("n", sorted(set(FIN_ROWS + [4])))
@pytest.mark.parametrize("C,nfold", SHAPES, ids=["512x1", "64x1", "64x12"])
def test_backward_coefficients_exact_tier(C, nfold, n, use_local):
    """bn_bwd_finalize_kernel on integer rows: every output bit for bit; every fold its own values; channel 2 sums to zero; `local`"""
    tag = "coef exact C=%d nfold=%d rows=%d %s" % (C, nfold, n, "local" if use_local else "plain")
    gen = _gen("coef exact", C, nfold, n)
    W = C * nfold
    totals = torch.randint(-4000, 4001, (2, nfold, C), generator=gen, device=DEV).double()
    totals[:, :, 2] = 0.0
    rows = br.spread_totals(totals.reshape(-1), n, gen).reshape(n, 2, W)
    local = torch.randint(-300, 301, (2 * W,), generator=gen, device=DEV).float() if use_local else None
    got, ref = _run_coef(tag, C, nfold, rows, 4096, _exact_bwd_stats(C, gen), True, local=local)
    assert float(got["coef"][1][2]) == 0.0 and float(got["coef"][2][2]) == 0.0, (tag, "the column with sum g = sum g r = 0")
    if nfold > 1:      # a transposed index would show: the folds of a channel differ, and so do the channels of a fold
        f = totals.reshape(2, nfold, C)[0]
        assert float((f[0] != f[1]).double().mean()) > 0.9 and float((f[:, 0] != f[:, 1]).double().mean()) > 0.9, tag
    if use_local:
        assert not torch.equal(ref["dbeta"], ref["s1"]), (tag, "local and global sums coincide")
    _report(tag)


@pytest.mark.parametrize("use_local", [False, True], ids=["plain", "local"])
@pytest.mark.parametrize("n", sorted(set(FIN_ROWS + [4])))
@pytest.mark.parametrize("C,nfold", SHAPES, ids=["512x1", "64x1", "64x12"])
def test_backward_coefficients_real_valued_tier(C, nfold, n, use_local):
    """bn_bwd_finalize_kernel on float32 sums (sum g, sum g r of 8 rows each) against float64 fed the same rows"""
    tag = "coef real C=%d nfold=%d rows=%d %s" % (C, nfold, n, "local" if use_local else "plain")
    gen = _gen("coef real", C, nfold, n)
    W = C * nfold
    sigma = torch.rand(C, generator=gen, device=DEV) * 1.5 + 0.5
    mu = torch.rand(C, generator=gen, device=DEV) * 2 * sigma
    mu[:8] = 100 * sigma[:8]
    r = torch.relu(torch.randn(n, 8, nfold, C, generator=gen, device=DEV) * sigma + mu)
    g = torch.randn(n, 8, nfold, C, generator=gen, device=DEV) * 1e-3
    rows = torch.stack([g.sum(1).reshape(n, W), (g * r).sum(1).reshape(n, W)], 1).contiguous()
    stats = torch.zeros(4, C, device=DEV)
    stats[0], stats[1] = mu, 1.0 / sigma
    stats[2] = stats[1] * (torch.rand(C, generator=gen, device=DEV) + 0.5)
    local = rows[0].reshape(-1).clone().contiguous() if use_local else None
    _run_coef(tag, C, nfold, rows, 8 * n * nfold, stats.contiguous(), False, local=local)
    _report(tag)


# ---- kinds 1 and 5: weight preparation -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights():
    return br.prep_weights(DEV)


def _params(o, w1=None, bn_g=None, bn_b=None):
    from contrastiveprosthetics_amd import _lib
    p = _lib.cp_params()
    for i in range(7):
        p.fc_w[i] = (w1 if (i == 0 and w1 is not None) else o["W%d" % (i + 1)]).data_ptr()
        p.fc_b[i] = o["b%d" % (i + 1)].data_ptr()
    p.last_w = o["Wp"].data_ptr()
    for l in range(9):
        if bn_g is not None:
            p.bn_g[l], p.bn_b[l] = bn_g[l].data_ptr(), bn_b[l].data_ptr()
    return p


def _image(tag, what, buf, ref, dtype):
    """every element of a prepared image against the float64 statement of its layout, rounded to T; the sentinel behind it"""
    n = ref.numel()
    want = ref.to(_torch_t(dtype))
    if dtype == BF16:
        assert torch.equal(want.double(), ref), (tag, what, "the image's values are not bf16 numbers")
    _same(tag, what, buf[:n].view(ref.shape), want)
    _untouched(tag, what, buf, n)


LAYER_C = [64, 64, 512, 512, 512, 512, 512, 512, 512]


@pytest.mark.parametrize("tier", ["exact", "real"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id_dtype)
def test_evaluation_prologue(dtype, tier):
    """kind 1: nine tables in one launch, eight folds in another.  exact: gamma from {0.5, 1, 2}, var from {0.25, 1, 4} under eps = 0,
    integer mean and beta, so s is a power of two from 0.25 to 4 and t a multiple of 1/4 -- the images and biases have one right
    answer; real: random tables under eps = 1e-5, the tables within the chain's bound (x = var + eps, sqrtf, division, product)."""
    from contrastiveprosthetics_amd import _lib
    tag = "eval prologue %s %s" % (_id_dtype(dtype), tier)
    gen = _gen("prologue", tier)
    o = _weights()
    pick = torch.tensor([0.5, 1.0, 2.0], device=DEV)
    g, b, m, v = [], [], [], []
    for C in LAYER_C:
        if tier == "exact":
            g.append(pick[torch.randint(0, 3, (C,), generator=gen, device=DEV)].contiguous())
            v.append((pick[torch.randint(0, 3, (C,), generator=gen, device=DEV)] ** 2).contiguous())
            m.append(torch.randint(-2, 3, (C,), generator=gen, device=DEV).float())
            b.append(torch.randint(-2, 3, (C,), generator=gen, device=DEV).float())
        else:
            g.append(torch.rand(C, generator=gen, device=DEV) + 0.5)
            v.append(torch.rand(C, generator=gen, device=DEV) * 4 + 1e-3)
            m.append(torch.randn(C, generator=gen, device=DEV) * 3)
            b.append(torch.randn(C, generator=gen, device=DEV))
    eps = 0.0 if tier == "exact" else EPS
    p = _params(o, bn_g=g, bn_b=b)
    bn = _lib.cp_bn_buffers()
    for l in range(9):
        bn.running_mean[l], bn.running_var[l] = m[l].data_ptr(), v[l].data_ptr()
    T = _torch_t(dtype)
    stats9 = [_buf(4 * C) for C in LAYER_C]
    wimg = [_buf(512 * (768 if i == 0 else 512), T) for i in range(7)] + [_buf(32 * 512, T)]
    bimg = [_buf(512) for _ in range(7)] + [_buf(16)]
    _launch(1, dtype, eps=eps, params=p, bn=bn, stats9=stats9, wimg=wimg, bimg=bimg)
    tables = []
    for l, C in enumerate(LAYER_C):
        ref = br.ref_running_stats(m[l], v[l], g[l], b[l], eps)
        _within(tag, "table %d" % l, stats9[l][:4 * C].view(4, C), ref, br.running_stats_bounds(ref))
        _same(tag, "table %d, mean" % l, stats9[l][:C], m[l])
        _untouched(tag, "table %d" % l, stats9[l], 4 * C)
        tables.append(ref)
    if tier == "exact":
        for i in range(8):
            s, t = tables[1 + i][2], tables[1 + i][3]
            assert torch.equal(s, s.bfloat16().double()) and torch.equal(t * 4, (t * 4).round()), (tag, "s or t is not exact")
            if i < 7:
                img, bias = br.ref_fold(o["W%d" % (i + 1)], o["b%d" % (i + 1)], s, t, 1 if i == 0 else 0)
            else:
                img, bias = br.ref_fold(o["Wp"], None, s, t, 0, rows_out=32)
                assert not bool(img[16:].any())
            Wi = (o["Wp"] if i == 7 else o["W%d" % (i + 1)]).double()
            ch = torch.arange(768, device=DEV) // 12 if i == 0 else torch.arange(512, device=DEV)
            _exact_stat(tag, "W t (layer %d)" % i, (Wi * t[ch]).T, 0.25)
            _image(tag, "image %d" % i, wimg[i], img, dtype)
            _same(tag, "bias %d" % i, bimg[i][:bias.numel()], bias)
            _untouched(tag, "bias %d" % i, bimg[i], bias.numel())
    else:
        for i in range(8):
            _untouched(tag, "image %d" % i, wimg[i], 32 * 512 if i == 7 else 512 * (768 if i == 0 else 512))
            _untouched(tag, "bias %d" % i, bimg[i], 16 if i == 7 else 512)
    _report(tag)


FOLD_CASES = [(0, 512, True, False), (0, 512, False, False), (0, 768, False, False), (1, 768, True, False), (1, 768, False, False),
              (1, 768, True, True), (1, 768, False, True)]


@pytest.mark.parametrize("mode,K,affine,coded", FOLD_CASES,
                         ids=["mode%d-K%d-%s-%s" % (c[0], c[1], "fold" if c[2] else "copy", "coded" if c[3] else "ternary") for c in FOLD_CASES])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id_dtype)
def test_fold_linear_during_training(dtype, mode, K, affine, coded):
    """kind 5, modes 0 and 1: fold_linear_kernel<T> on 512 blocks, with and without the previous BatchNorm's affine; the coded W of
    mode 1 carries (c, w) in every entry"""
    tag = "fold %s mode %d K=%d %s %s" % (_id_dtype(dtype), mode, K, "fold" if affine else "copy", "coded" if coded else "ternary")
    gen = _gen("fold", mode, K, affine, coded)
    o = _weights()
    W = br.coded_w1(DEV, dtype == BF16) if coded else (o["W1"] if K == 768 else o["W2"])
    b = o["b1"]
    C = 64 if mode == 1 else K
    s = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (C,), generator=gen, device=DEV)].contiguous() if affine else None
    t = torch.randint(-2, 3, (C,), generator=gen, device=DEV).float() if affine else None
    img, bias = br.ref_fold(W, b, s, t, mode)
    if affine:
        ch = torch.arange(K, device=DEV) // 12 if mode == 1 else torch.arange(K, device=DEV)
        _exact_stat(tag, "W t", (W.double() * t.double()[ch]).T, 1.0)
    out_w, out_b = _buf(512 * K, _torch_t(dtype)), _buf(512)
    _launch(5, dtype, mode=mode, K=K, W=W, b=b, s=s, t=t, wimg=[out_w], bimg=[out_b])
    _image(tag, "the image", out_w, img, dtype)
    _same(tag, "the bias", out_b[:512], bias)
    _untouched(tag, "the bias", out_b, 512)
    _report(tag)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id_dtype)
def test_fold_copies_of_the_dropout_forward(dtype):
    """kind 5, mode 2: the four-job fold_copy_batch_kernel<T> (fc5..fc7 and the projection, whose job has rows_out = 32 < 512 blocks)"""
    tag = "fold copies %s" % _id_dtype(dtype)
    o = _weights()
    T = _torch_t(dtype)
    wimg = [None] * 4 + [_buf(512 * 512, T) for _ in range(3)] + [_buf(32 * 512, T)]
    bimg = [None] * 4 + [_buf(512) for _ in range(3)] + [_buf(16)]
    _launch(5, dtype, mode=2, params=_params(o), wimg=wimg, bimg=bimg)
    for i in (4, 5, 6):
        _image(tag, "image %d" % i, wimg[i], o["W%d" % (i + 1)].double(), dtype)
        _same(tag, "bias %d" % i, bimg[i][:512], o["b%d" % (i + 1)])
        _untouched(tag, "bias %d" % i, bimg[i], 512)
    img, bias = br.ref_fold(o["Wp"], None, None, None, 0, rows_out=32)
    _image(tag, "the projection's image, rows 16..31 zero", wimg[7], img, dtype)
    _same(tag, "the projection's bias", bimg[7][:16], bias)
    _untouched(tag, "the projection's bias", bimg[7], 16)


@pytest.mark.parametrize("coded", [False, True], ids=["ternary", "coded"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id_dtype)
def test_weight_transposes_of_the_backward(dtype, coded):
    """kind 5, mode 3: the eight-job transpose_w_batch_kernel<T>: fc1 in the order k' = w * 64 + c, the projection into 64 columns"""
    tag = "transposes %s %s" % (_id_dtype(dtype), "coded" if coded else "ternary")
    o = _weights()
    w1 = br.coded_w1(DEV, dtype == BF16) if coded else o["W1"]
    T = _torch_t(dtype)
    wimg = [_buf(512 * (768 if i == 0 else 512), T) for i in range(7)] + [_buf(512 * 64, T)]
    _launch(5, dtype, mode=3, params=_params(o, w1=w1), wimg=wimg)
    _image(tag, "fc1^T", wimg[0], br.ref_transpose(w1, 1, 512), dtype)
    for i in range(1, 7):
        _image(tag, "fc%d^T" % (i + 1), wimg[i], br.ref_transpose(o["W%d" % (i + 1)], 0, 512), dtype)
    ref = br.ref_transpose(o["Wp"], 0, 64)
    assert not bool(ref[:, 16:].any())
    _image(tag, "the projection's transpose, columns 16..63 zero", wimg[7], ref, dtype)
