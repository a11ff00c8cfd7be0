"""The launches of the 8-bit fc path (dtype="fp8", csrc/fp8.cuh) on their own, one sequence at a time through cp_debug_fp8, at
tolerance ZERO and ragged row counts.

What runs (include/cpnative.h, cp_debug_fp8; the launch functions, grids and row splits are the step's own, csrc/fp8.cuh and
csrc/encoder_api.cuh), on caller buffers and a caller scale table (1,024 bytes laid out as Fp8State: e[64], amax[64], init):

    kind 0   gemm_ws8_kernel<512 | 768, STATS | evaluation>   -> C[M][512] e4m3, partials[rows][2][512], amax
    kind 1   gemm_wsd8_kernel<0>, F = 512 (coef_mod 512) and F = 768 (coef_mod 64) -> C[M][F] e5m2, partials[rows][F], amax
    kind 2   gemm_wsd8_kernel<1>, F = 512                      -> C e5m2, partials[rows][2][512], amax
    kind 3   gemm_tn8_kernel + reduce_slabs_kernel<bf16>: single (Q = 512, 64 splits), single (Q = 768, 40 splits), paired (32 each)
             -> bf16 slabs[S][512][Q], dW[512][Q]
    kind 4   bn_dropout_apply8_kernel                          -> u[M][512] e4m3, amax
    kind 5   bn_relu_bwd8_kernel, in place                     -> g[M][512] e5m2, partials[grid][512], amax
    kind 6   proj_dgrad8_kernel, with and without dropout      -> C[M][512] e5m2, partials[rows][512], amax
    kind 7   fold_linear8_kernel (mode 0, and 1 = fc1's order k' = w*64 + c), transpose_w8_batch_kernel (one job)
             -> weight bytes, scale bytes, bias in output units
    kind 8   fp8_update_scales_kernel                          -> the table

Why zero (the recipe of tests/test_gpu_fc_gemm_exact.py in 8 bits): small integers times powers of two are exact in e4m3 and e5m2,
every tensor scale and weight-row scale is a power of two, and rounding an exactly known accumulator to e4m3 or e5m2 is a function.
Gradients (e5m2) are {-2, 0, 2} with +-2 at probability 1/16 each, weights (e4m3) ternary with +-1 at 1/8 each (every row and column
holds a non-zero weight, asserted), weight-row scale bytes 127 + {-1, 0, 1} (three forward features at 127 + 3, so that outputs pass
448: the clamp and amax), activations relu(randint(-2, 4)) 2^r with r in {0, 1, -1} through e[t_r], bias, cb, cz and shift small
integers, ca and scale from {0.5, 1, 2}, dropout at p = 0.5 (threshold 32768, 1 / (1 - p) = 2).  The reference is the same
operation in float64 torch, rounded with x.clamp(-448, 448).to(float8_e4m3fn) / x.clamp(-57344, 57344).to(float8_e5m2) (nearest
even on exact inputs, asserted in test_the_reference_rounds_to_nearest_even); bytes are compared through .view(uint8).

Preconditions, asserted on the reference before anything is compared (`_exact_acc`, `_exact_f32`, `_worker_sums`): every
accumulator and epilogue intermediate is a float32, every accumulator a multiple of its step below 2^24 steps, every per-worker or
per-block column sum likewise, every slab entry known exactly before its bf16 rounding.  Each case prints the largest it saw (-s).

Planted edges: feature 13 of the data gradients carries a weight-row scale of 2^13 (kinds 1, 2) or a coefficient ca of 2^15 / 2^16
(kinds 5, 6), so that outputs lie beyond 57,344 and must store 0x7B / 0xFB -- these epilogues rely on the saturating conversion
mode, not on a clamp -- and feature 13 of kind 4 a BatchNorm scale of 512 (beyond 448: 0x7E / 0xFE); feature 21 of kind 2 has
scale = 0 (the branch |s| <= 1e-30: sum g r = mean sum g); column 9 of R is non-positive with cz = 1024 (kinds 1, 5, 6: the byte
0, and the 1,024 never reaches amax); negative pre-activations of kind 0 store +0; kind 7 has an all-zero weight row, rows whose
maximum is 448 2^k and one float above, and scale bytes at the clamps 1 and 254; kind 8 a fresh table with n_windows 1, 2^k, 2^k + 1
and maxima at 224 2^-e, 1024 2^-e and one ulp above.

What is compared (torch.equal): every output byte below M and the sentinel bytes (0x7F, a NaN in both formats) of the guard rows
behind M; amax[t_out] as the float bits of the reference's largest magnitude before clamping (kind 0: largest accumulator), all other
words of the table unchanged; *rows_out = min(tiles, workers) and EACH partial row against the sums over that worker's rows (kind 0:
clamped values before rounding and their squares; kinds 1, 2, 5, 6: values as stored, in true units), the rows of workers without a
tile and the floats behind still the sentinel; kind 3: each slab against the bf16 rounding of that split's product, dW against the
float64 sum of the rounded slabs times 2^-(ex + ey), both problems of a paired launch; kinds 4 and 6: the mask against numpy's
restatement of the hash (tools/dropout_hash_check.py) element by element, kept share within 6 binomial standard deviations of 0.5.

Row counts, the smallest at which each piece of control flow is first taken.  Weight-stationary kernels, T-row tiles and W workers,
worker w runs tiles w, w + W, ..: 1, T - 1, T, T + 1, T W - 1, T W, and T W (n - 1) + 1 for n = 2 .. NBUF + 2 (worker 0 runs n
tiles, the last with one live row: every branch of the counted waits, both parities of the ping-pong tail, a ring that wraps):
gemm_ws8<512> T 64, W 128, NBUF 3, up to 32,769; gemm_ws8<768> and gemm_wsd8 at F = 512 T 32, W 128, NBUF 4, up to 20,481;
gemm_wsd8<0> at F = 768 T 32, W 80, up to 12,801; proj_dgrad8 T 32, W 256, two R buffers, up to 16,385.  gemm_tn8 (64-row stages, ring
of 4, rows per split rounded to 64): 1, 63, 64, 65, one row past 64 target s for s = 1 .. 5 stages per split (vmcnt(0), (4), (8), the
ring wraps at 5) and one M whose last split ends in the middle of a stage.  Streaming kernels (8 rows per block, grid cap 512, four
rows in flight): 1, 7, 8, 9, 4,095 .. 4,097 (the cap), 12,288 (tail alone), 12,289 (one unrolled batch), 16,383 .. 16,385 (the
unrolled loop alone, and with a tail), 20,481.  The operands hold live data behind row M."""
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
M_MAX = 32769
M_ALLOC = M_MAX + 160
GUARD_ROWS = 160
GUARD_FLOATS = 8192
SENTINEL8 = 0x7F                        # NaN in e4m3 and in e5m2
SENTINEL16 = 0x7FA5                     # a bf16 NaN
SENTINEL32 = 0x7FC0BEEF                 # a float32 NaN
DP_THRESH, DP_INV_KEEP, DP_KEY = 32768, 2.0, 0x5EED1234
F8_NT = 64
T_IN, T_R, T_OUT, T_IN2, T_R2 = 17, 5, 40, 22, 9          # scale-table ids of a launch: nothing but the arguments ties a tensor to an id
SAT, ZERO_SCALE, NONPOS = 13, 21, 9                       # planted features
EXPS = [(0, 0), (1, -1), (-1, 1)]                         # (e[t_r], e[t_out]), cycled over the row counts of a table


def _ws_rows(T, W, nbuf):
    return [1, T - 1, T, T + 1, T * W - 1, T * W] + [T * W * (n - 1) + 1 for n in range(2, nbuf + 3)]


WS512_M = _ws_rows(64, 128, 3)
WS768_M = _ws_rows(32, 128, 4)
WSD512_M = _ws_rows(32, 128, 4)
WSD768_M = _ws_rows(32, 80, 4)
PROJ_M = [1, 31, 32, 33, 8191, 8192, 8193, 16385]         # 256 workers, two R buffers: the third tile wraps
TN_M = {64: [1, 63, 64, 65] + [64 * 64 * s + 1 for s in range(1, 6)] + [5087],
        40: [1, 65] + [64 * 40 * s + 1 for s in range(1, 6)] + [3000],
        32: [1, 65] + [64 * 32 * s + 1 for s in range(1, 6)] + [2500]}
STREAM_M = [1, 7, 8, 9, 4095, 4096, 4097, 12288, 12289, 16383, 16384, 16385, 20481]


# ---- rounding --------------------------------------------------------------------------------------------------------------------
def e4m3(x):
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def e5m2(x):
    return x.float().clamp(-57344.0, 57344.0).to(torch.float8_e5m2)


def test_the_reference_rounds_to_nearest_even():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    assert e4m3(t(17, 19, 25, 465, -465, -3)).float().tolist() == [16, 20, 24, 448, -448, -3]
    assert e5m2(t(9, 11, 60000, -70000, 1e6)).float().tolist() == [8, 12, 57344, -57344, 57344]
    assert e5m2(t(60000, -60000)).view(torch.uint8).tolist() == [0x7B, 0xFB]
    assert e4m3(t(3072, -3072, -0.0)).view(torch.uint8).tolist() == [0x7E, 0xFE, 0x80]


# ---- operands --------------------------------------------------------------------------------------------------------------------
def _ternary(shape, gen, n):
    """1 and -1 with probability 1 / n each, else 0"""
    u = torch.randint(0, n, shape, generator=gen, device=DEV)
    return (u == 0).float() - (u == 1).float()


@functools.lru_cache(maxsize=None)
def _operands():
    """the recipe of the module docstring, made once: slices [:M] serve every case"""
    gen = torch.Generator(device=DEV).manual_seed(80816)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen, device=DEV).float()
    pick = torch.tensor([0.5, 1.0, 2.0], device=DEV)
    o = {}
    o["act"] = torch.relu(ri(-2, 4, M_ALLOC, 768))                    # saved activations, true units
    R = o["act"].clone()
    R[:, NONPOS] = -R[:, NONPOS]
    o["R"] = R                                                        # what the data gradients read: column 9 is never positive
    o["G"] = 2.0 * _ternary((M_ALLOC, 512), gen, 16)                  # gradients as stored
    o["G2"] = 2.0 * _ternary((M_ALLOC, 512), gen, 16)
    o["Gw"], o["Gw2"] = o["G"].clone(), o["G2"].clone()               # the weight gradients' X: row 0 of the product sums 6 y over one
    o["Gw"][:, 0], o["Gw2"][:, 0] = 6.0, -6.0                         # sign, so that from 128 rows per split on its slab entries need more than bf16's 8 bits
    u = ri(-2, 4, M_ALLOC, 512) * (torch.rand(M_ALLOC, 512, generator=gen, device=DEV) < 0.5).float()
    o["u"] = u                                                        # a dropout output: its zeros are the mask
    o["Wf"] = _ternary((512, 768), gen, 8)
    o["Wd"] = _ternary((768, 512), gen, 8)
    for name, w in (("Wf[:, :512]", o["Wf"][:, :512]), ("Wf", o["Wf"]), ("Wd[:512]", o["Wd"][:512]), ("Wd", o["Wd"])):
        assert bool((w != 0).any(0).all()) and bool((w != 0).any(1).all()), "a row or column of %s holds no non-zero weight" % name
    scf = 127 + ri(-1, 2, 512)
    big = o["Wf"][:, :512].sum(1).topk(3).indices                     # (the three features with the most positive weights: their outputs pass 448)
    scf[big] = 127 + 3
    scd = 127 + ri(-1, 2, 768)
    scd[SAT] = 127 + 13
    o["scf"], o["scd"] = scf.to(torch.uint8), scd.to(torch.uint8)
    o["bias"], o["bias_step"] = ri(-3, 4, 512), torch.ones(512, device=DEV)
    o["bias"][big] = torch.tensor([0.0, 16.0, -16.0], device=DEV)     # (multiples of 16: these features' sums of squares run in steps of 16^2 2^2r)
    o["bias_step"][big] = 16.0
    coef = torch.stack([pick[ri(0, 3, 512).long()], ri(-1, 2, 512), ri(-2, 3, 512)])
    coef[2, NONPOS] = 1024.0
    coef[0, SAT] = coef[0, 64 + SAT] = 2.0
    o["coef"] = coef.contiguous()
    o["coef64"] = coef[:, 64:128].contiguous()                        # fc1's gradient into the conv stack: 64 channels, 12 positions
    c5, c6 = coef.clone(), coef.clone()
    c5[0, SAT], c6[0, SAT] = 2.0 ** 15, 2.0 ** 16
    o["coef5"], o["coef6"] = c5.contiguous(), c6.contiguous()
    stats = torch.stack([ri(-2, 3, 512), torch.ones(512, device=DEV), pick[ri(0, 3, 512).long()], ri(-2, 3, 512)])     # mean, invstd, scale, shift
    o["stats4"] = stats.clone()
    o["stats4"][2, SAT] = 512.0
    stats[2, ZERO_SCALE] = 0.0
    o["stats2"] = stats.contiguous()
    o["stats4"] = o["stats4"].contiguous()
    dz = torch.zeros(M_ALLOC, 64, device=DEV)
    dz[:, :16] = _ternary((M_ALLOC, 16), gen, 16)
    o["dz"] = dz
    wp = torch.zeros(512, 64, device=DEV)
    wp[:, :16] = _ternary((512, 16), gen, 4)
    assert bool((wp != 0).any(1).all()), "a feature of the projection never sees a non-zero weight"
    o["Wp_t"] = wp
    return o


@functools.lru_cache(maxsize=None)
def _bytes(name, exp, fmt):
    """operand `name` times 2^exp as e4m3 / e5m2 bytes: exact, asserted"""
    stored = _operands()[name].double() * 2.0 ** exp
    q = e4m3(stored) if fmt == 4 else e5m2(stored)
    assert torch.equal(q.double(), stored), "the 8-bit form of %s is not exact" % name
    return q.view(torch.uint8).contiguous()


@functools.lru_cache(maxsize=None)
def _bf16(name):
    return _operands()[name].bfloat16().contiguous()


@functools.lru_cache(maxsize=None)
def _keep():
    """the kernels' keep decision for element (m, f) of an [.][512] tensor, from the numpy restatement of csrc/common.cuh
    dropout_quad: quad index (m * 512 + f) >> 2, draw f & 3"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dropout_hash_check as dh
    n = max(STREAM_M + PROJ_M)
    idx = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(128) + np.arange(128, dtype=np.uint64)[None, :]
    a, b = dh.quad(idx, np.uint64(DP_KEY))
    draws = np.stack(dh.draws(a, b), axis=-1).reshape(n, 512)
    keep = torch.from_numpy(draws >= DP_THRESH).to(DEV)
    for M in sorted(set(STREAM_M + PROJ_M)):
        if M >= 31:
            cnt = M * 512
            share = float(keep[:M].sum()) / cnt
            assert abs(share - 0.5) <= 6 * (0.25 / cnt) ** 0.5, ("kept share", M, share)
    return keep


# ---- buffers, the table, the launch ------------------------------------------------------------------------------------------------
def _buf(n, dtype=torch.float32):
    """n elements and a guard behind them, all sentinel"""
    t = torch.empty(n + GUARD_FLOATS, dtype=dtype, device=DEV)
    if dtype == torch.float32:
        t.view(torch.int32).fill_(SENTINEL32)
    elif dtype == torch.bfloat16:
        t.view(torch.int16).fill_(SENTINEL16)
    else:
        t.fill_(SENTINEL8)
    return t


def _sentinel_of(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32), SENTINEL32
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16), SENTINEL16
    return t, SENTINEL8


def _untouched(tag, what, t, n):
    tail, s = _sentinel_of(t[n:])
    assert torch.equal(tail, torch.full_like(tail, s)), (tag, "elements behind %s were written" % what)


def _out_rows(M, F):
    """[M + GUARD_ROWS][F] bytes, all sentinel"""
    return torch.full((M + GUARD_ROWS, F), SENTINEL8, dtype=torch.uint8, device=DEV)


def _t(e):
    """a scale table with e[t] set for the ids a launch reads, amax zero, init 1; the other exponents hold a value no launch may read"""
    t = torch.zeros(256, dtype=torch.int32, device=DEV)
    t[:F8_NT] = 77
    for k, v in e.items():
        t[k] = v
    t[128] = 1
    return t


def _table_after(tag, table, before, t_out, amax):
    """amax[t_out] holds the float bits of `amax` (None or 0: untouched), every other word is what it was"""
    want = before.clone()
    if t_out is not None and amax is not None and amax > 0:
        want[F8_NT + t_out] = int(np.float32(amax).view(np.int32))
    got = table.cpu()
    if not torch.equal(got, want.cpu()):
        bad = (got != want.cpu()).nonzero().flatten().tolist()
        raise AssertionError((tag, "scale table words %s: got %s, want %s" % (bad, [hex(int(got[i]) & 0xFFFFFFFF) for i in bad],
                                                                                [hex(int(want[i]) & 0xFFFFFFFF) for i in bad])))


def _launch(kind, M, table, mode=0, **kw):
    from contrastiveprosthetics_amd import _lib
    d = _lib.cp_debug_fp8_args()
    d.kind, d.mode, d.M, d.K, d.F, d.coef_mod = kind, mode, M, 512, 512, 512
    d.t_in, d.t_r, d.t_out, d.t_in2, d.t_r2 = T_IN, T_R, T_OUT, T_IN2, T_R2
    d.state = table.data_ptr()
    for name, v in kw.items():
        setattr(d, name, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rows = ctypes.c_int32(-1)
    d.rows_out = ctypes.pointer(rows)
    _lib.check(_lib.load().cp_debug_fp8(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "cp_debug_fp8")
    torch.cuda.synchronize()
    return rows.value


# ---- the preconditions of "tolerance zero", asserted on the reference ------------------------------------------------------
SEEN = {}


def _note(tag, name, v):
    SEEN.setdefault(tag, {})[name] = float(v)


def _exact_f32(tag, name, x):
    """an epilogue intermediate is a float32: the kernel's float32 operation that forms it rounds nothing"""
    assert torch.equal(x, x.float().double()), (tag, name, "not a float32")
    _note(tag, "max |%s|" % name, x.abs().max())


def _exact_acc(tag, name, a, b, step, extra=None):
    """every accumulator of a @ b (plus |extra|) is exact in float32 in any order: a multiple of `step` (per column, or one number) and
    sum |a| |b| below 2^24 steps"""
    q = a.abs() @ b.abs()
    if extra is not None:
        q = q + extra.abs()
    q = q / step
    assert torch.equal(q, q.round()), (tag, name)
    top = float(q.max())
    assert top < 2 ** 24, (tag, name, top)
    _note(tag, "sum |%s| / step" % name, top)


def _worker_sums(tag, name, terms, step, worker, n_workers):
    """the sums of `terms` over the rows of each worker: [n_workers][F] float64.  Exact in float32 in any order and grouping: every
    term is a multiple of `step` (per column, or one number) and even a worker's column sum of |term| stays below 2^24 steps"""
    q = terms / step
    assert torch.equal(q, q.round()), (tag, name)
    mag = torch.zeros(n_workers, terms.shape[1], dtype=torch.float64, device=terms.device).index_add_(0, worker, q.abs())
    top = float(mag.max())
    assert top < 2 ** 24, (tag, name, top)
    _note(tag, "worker sum |%s| / step" % name, top)
    return torch.zeros(n_workers, terms.shape[1], dtype=torch.float64, device=terms.device).index_add_(0, worker, terms)


def _report(tag):
    print("\n[fp8_exact] %s: %s (2^24 = 16777216)" % (tag, ", ".join("%s %g" % kv for kv in SEEN.get(tag, {}).items())))


def _where(got, ref):
    bad = got != ref
    rows = bad.any(1).nonzero().flatten()
    cols = bad.any(0).nonzero().flatten()
    r0, c0 = (int(x) for x in bad.nonzero()[0])
    return "%d elements differ; rows %s .. %s (%d rows), 32-row tiles %s, columns %s .. %s (%d columns); [%d][%d]: got %r, want %r" % (
        int(bad.sum()), rows[:8].tolist(), rows[-3:].tolist(), rows.numel(), torch.unique(rows // 32)[:12].tolist(),
        cols[:8].tolist(), cols[-3:].tolist(), cols.numel(), r0, c0, got[r0, c0].item(), ref[r0, c0].item())


def _same(tag, what, got, ref):
    if got.dim() == 1:
        got, ref = got[None], ref[None]
    if got.dtype != torch.uint8:
        got, ref = got.double(), ref.double()
    assert torch.equal(got, ref), (tag, what, _where(got, ref))


def _same_bytes(tag, out, M, ref8):
    _same(tag, "output bytes", out[:M], ref8.view(torch.uint8))
    guard = out[M:]
    assert torch.equal(guard, torch.full_like(guard, SENTINEL8)), (tag, "rows behind M were written")


def _workers(M, T, W):
    """worker of each row (tiles w, w + W, ..) and the number of partial rows: min(tiles, workers)"""
    m = torch.arange(M, device=DEV)
    return (m // T) % W, min(-(-M // T), W)


def _same_partials(tag, part, n_rows, width, ref_rows):
    """each partial row against the sums of its worker's rows; behind them the sentinel (workers without a tile write nothing)"""
    got = part[:n_rows * width].view(n_rows, width)
    _same(tag, "partial rows", got, ref_rows[:n_rows].reshape(n_rows, width))
    _untouched(tag, "partial row %d" % (n_rows - 1), part, n_rows * width)


# ---- kind 0: the forward ---------------------------------------------------------------------------------------------------------
def ref_forward(tag, K, M, r):
    o = _operands()
    A = o["act"][:M, :K].double() * 2.0 ** r
    W = o["Wf"][:, :K].double()
    sc = 2.0 ** (o["scf"].double() - 127)
    b = o["bias"].double()
    step = torch.minimum(sc * 2.0 ** r, o["bias_step"].double())
    _exact_acc(tag, "A W", A, W.T * sc, step, b)
    acc = (A @ W.T) * sc + b
    v = acc.clamp(0.0, 448.0)
    assert bool((acc < 0).any()), (tag, "no negative pre-activation")
    if M >= 8191 and r >= 0:
        assert bool((acc > 448).any()), (tag, "no output beyond 448")
    if M >= 64:
        _note(tag, "share of outputs e4m3 rounds", float((e4m3(v).double() != v).double().mean()))
    T = 64 if K == 512 else 32
    worker, n_rows = _workers(M, T, 128)
    s1 = _worker_sums(tag, "v", v, step, worker, 128)
    s2 = _worker_sums(tag, "v^2", v * v, step * step, worker, 128)
    return dict(C=e4m3(v), amax=float(acc.max()), rows=torch.stack([s1, s2], 1), n_rows=n_rows)


def _check_forward(K, M, r, stats):
    tag = "forward K=%d M=%d r=%d %s" % (K, M, r, "stats" if stats else "evaluation")
    ref = ref_forward(tag, K, M, r)
    o = _operands()
    A = _bytes("act", r, 4)[:, :K].contiguous() if K == 512 else _bytes("act", r, 4)
    W = e4m3(o["Wf"][:, :K]).view(torch.uint8).contiguous()
    table = _t({T_OUT: 3})
    before = table.clone()
    C, part = _out_rows(M, 512), _buf(128 * 2 * 512)
    rows = _launch(0, M, table, K=K, A=A, W=W, wsc=o["scf"], bias=o["bias"], C=C, partials=part if stats else None)
    _same_bytes(tag, C, M, ref["C"])
    assert not bool(((C[:M] == 0x80)).any()), (tag, "a negative zero was stored")
    _table_after(tag, table, before, T_OUT, ref["amax"])
    if stats:
        assert rows == ref["n_rows"], (tag, "partial rows", rows, ref["n_rows"])
        _same_partials(tag, part, rows, 1024, ref["rows"])
    else:
        assert rows == 0, (tag, rows)
        _untouched(tag, "partials (evaluation form)", part, 0)
    _report(tag)


@pytest.mark.parametrize("M", WS512_M)
def test_forward_512_is_exact(M):
    _check_forward(512, M, EXPS[WS512_M.index(M) % 3][0], True)


@pytest.mark.parametrize("M", WS768_M)
def test_forward_768_is_exact(M):
    _check_forward(768, M, EXPS[WS768_M.index(M) % 3][0], True)


@pytest.mark.parametrize("K,M", [(512, 65), (512, 16385), (768, 33), (768, 12289)])
def test_forward_without_sums_is_exact(K, M):
    _check_forward(K, M, 0, False)


# ---- kinds 1 and 2: the data gradients -------------------------------------------------------------------------------------------
def _dgrad_acc(tag, F, M):
    o = _operands()
    G = o["G"][:M].double()
    Wt = o["Wd"][:F].double()
    sc = 2.0 ** (o["scd"][:F].double() - 127)
    _exact_acc(tag, "G W", G, Wt.T * sc, sc)
    return (G @ Wt.T) * sc


def ref_dgrad_bn(tag, F, M, e_r, e_o):
    o = _operands()
    acc = _dgrad_acc(tag, F, M)
    rv = o["R"][:M, :F].double() * 2.0 ** e_r
    mod = 512 if F == 512 else 64
    ca, cb, cz = (c.double()[torch.arange(F, device=DEV) % mod] for c in (o["coef"] if F == 512 else o["coef64"]))
    so, sr = 2.0 ** e_o, 2.0 ** (e_o - e_r)
    inner = (cb * sr) * rv + cz * so
    y = torch.where(rv > 0, (ca * so) * acc + inner, torch.zeros_like(acc))
    _exact_f32(tag, "cb r + cz", inner)
    _exact_f32(tag, "y", y)
    return y, 512 if F == 512 else 64


def _stored_e5m2(tag, y, big):
    C = e5m2(y)
    if big:
        sat = y.abs() > 57344
        assert bool((y > 57344).any()) and bool((y < -57344).any()), (tag, "no output beyond 57,344 on both sides")
        assert set(C.view(torch.uint8)[sat].tolist()) == {0x7B, 0xFB}, tag
        _note(tag, "outputs beyond 57344", float(sat.sum()))
    return C


@pytest.mark.parametrize("F,M", [(512, M) for M in WSD512_M] + [(768, M) for M in WSD768_M])
def test_data_gradient_with_batchnorm_backward_is_exact(F, M):
    table_m = WSD512_M if F == 512 else WSD768_M
    e_r, e_o = EXPS[table_m.index(M) % 3]
    tag = "dgrad<0> F=%d M=%d e_r=%d e_o=%d" % (F, M, e_r, e_o)
    o = _operands()
    y, mod = ref_dgrad_bn(tag, F, M, e_r, e_o)
    Cq = _stored_e5m2(tag, y, M >= 4096)
    assert not bool(Cq.view(torch.uint8)[:, NONPOS].any()), (tag, "column 9 of the reference is not the byte 0")
    W = 128 if F == 512 else 80
    worker, n_rows = _workers(M, 32, W)
    ref_rows = _worker_sums(tag, "C as stored", Cq.double(), 2.0 ** (e_o - 1), worker, W) * 2.0 ** -e_o
    table = _t({T_R: e_r, T_OUT: e_o})
    before = table.clone()
    R8 = _bytes("R", e_r, 4)
    R8 = R8[:, :512].contiguous() if F == 512 else R8
    C, part = _out_rows(M, F), _buf(W * F)
    rows = _launch(1, M, table, F=F, coef_mod=mod, A=_bytes("G", 0, 5), W=e4m3(o["Wd"][:F]).view(torch.uint8).contiguous(), wsc=o["scd"],
                   R=R8, coef=o["coef"] if F == 512 else o["coef64"], C=C, partials=part)
    _same_bytes(tag, C, M, Cq)
    _table_after(tag, table, before, T_OUT, float(y.abs().max()))
    assert rows == n_rows, (tag, "partial rows", rows, n_rows)
    _same_partials(tag, part, rows, F, ref_rows)
    _report(tag)


@pytest.mark.parametrize("M", WSD512_M)
def test_data_gradient_behind_a_dropout_is_exact(M):
    e_r, e_o = EXPS[WSD512_M.index(M) % 3]
    tag = "dgrad<1> M=%d e_r=%d e_o=%d" % (M, e_r, e_o)
    o = _operands()
    acc = _dgrad_acc(tag, 512, M)
    rv = o["u"][:M].double() * 2.0 ** e_r
    y = torch.where(rv != 0, acc * (DP_INV_KEEP * 2.0 ** e_o), torch.zeros_like(acc))
    _exact_f32(tag, "y", y)
    Cq = _stored_e5m2(tag, y, M >= 4096)
    st = Cq.double()
    worker, n_rows = _workers(M, 32, 128)
    s1 = _worker_sums(tag, "g as stored", st, 2.0 ** e_o, worker, 128) * 2.0 ** -e_o
    s2 = _worker_sums(tag, "g u as stored", st * rv, 2.0 ** (e_o + e_r), worker, 128) * 2.0 ** (-e_o - e_r)
    mean, _, s, t = (x.double() for x in o["stats2"])
    half, st1 = s2 / DP_INV_KEEP, t * s1
    for name, x in (("sum g u (1 - p)", half), ("t sum g", st1), ("their difference", half - st1), ("mean sum g", mean * s1)):
        _exact_f32(tag, name, x)
    gr = torch.where(s.abs() > 1e-30, (half - st1) / torch.where(s == 0, torch.ones_like(s), s), mean * s1)
    _exact_f32(tag, "sum g r", gr)
    assert float(s[ZERO_SCALE]) == 0.0 and (M < 4096 or bool((s1[:, ZERO_SCALE] * mean[ZERO_SCALE] != 0).any())), (tag, "the zero-scale feature shows nothing")
    table = _t({T_R: e_r, T_OUT: e_o})
    before = table.clone()
    C, part = _out_rows(M, 512), _buf(128 * 2 * 512)
    rows = _launch(2, M, table, A=_bytes("G", 0, 5), W=e4m3(o["Wd"][:512]).view(torch.uint8).contiguous(), wsc=o["scd"], R=_bytes("u", e_r, 4),
                   bn_stats=o["stats2"], C=C, partials=part, dp_inv_keep=DP_INV_KEEP)
    _same_bytes(tag, C, M, Cq)
    _table_after(tag, table, before, T_OUT, float(y.abs().max()))
    assert rows == n_rows, (tag, "partial rows", rows, n_rows)
    _same_partials(tag, part, rows, 1024, torch.stack([s1, gr], 1))
    _report(tag)


# ---- kind 3: the weight gradient -------------------------------------------------------------------------------------------------
def _tn_split(M, target):
    rps = -(-(-(-M // target)) // 64) * 64
    return rps, -(-M // rps)


def _ref_wgrad(tag, X, Y, M, rps, S, ex, ey):
    raw = []
    for s in range(S):
        x, y = X[s * rps:min(M, (s + 1) * rps)], Y[s * rps:min(M, (s + 1) * rps)]
        _exact_acc(tag, "X^T Y", x.T, y, 2.0 ** min(ey, 0))
        raw.append(x.T @ y)
    raw = torch.stack(raw)
    slabs = raw.float().bfloat16()
    total = slabs.double().sum(0)
    q = slabs.double().abs().sum(0) / 2.0 ** min(ey, 0)
    assert torch.equal(q, q.round()) and float(q.max()) < 2 ** 24, (tag, "the sum of the slabs is not exact in float32")
    rounded = slabs.double() != raw
    assert rps < 128 or M < rps or bool(rounded.any()), (tag, "bf16 rounds no slab entry")
    _note(tag, "share of slab entries bf16 rounds", float(rounded.double().mean()))
    return slabs, total * 2.0 ** -(ex + ey)


def _check_wgrad(Q, paired, M):
    target = 32 if paired else (64 if Q == 512 else 40)
    rps, S = _tn_split(M, target)
    ex, ey = EXPS[TN_M[target].index(M) % 3]
    ex2, ey2 = ey, ex
    tag = "wgrad Q=%d %s M=%d rows/split=%d S=%d" % (Q, "paired" if paired else "single", M, rps, S)
    o = _operands()
    X, Y = o["Gw"][:M].double(), o["act"][:M, :Q].double() * 2.0 ** ey            # as stored: the product is in stored units
    slabs_ref, dW_ref = _ref_wgrad(tag, X, Y, M, rps, S, ex, ey)
    Y8 = _bytes("act", ey, 4)
    Y8 = Y8[:, :512].contiguous() if Q == 512 else Y8
    table = _t({T_IN: ex, T_R: ey, T_IN2: ex2, T_R2: ey2})
    before = table.clone()
    slabs, dW = _buf(S * 512 * Q, torch.bfloat16), _buf(512 * Q)
    kw = {}
    if paired:
        X2, Y2 = o["Gw2"][:M].double(), o["act"][:M, 256:].double() * 2.0 ** ey2
        slabs2_ref, dW2_ref = _ref_wgrad(tag + " (second)", X2, Y2, M, rps, S, ex2, ey2)
        slabs2, dW2 = _buf(S * 512 * 512, torch.bfloat16), _buf(512 * 512)
        kw = dict(A2=_bytes("Gw2", 0, 5), R2=_bytes("act", ey2, 4)[:, 256:].contiguous(), partials2=slabs2, C2=dW2)
    rows = _launch(3, M, table, mode=1 if paired else 0, F=Q, A=_bytes("Gw", 0, 5), R=Y8, partials=slabs, C=dW, **kw)
    assert rows == S, (tag, "splits", rows, S)
    _table_after(tag, table, before, None, None)
    for name, sl, sl_ref, d, d_ref, q in [("", slabs, slabs_ref, dW, dW_ref, Q)] + ([(" (second)", slabs2, slabs2_ref, dW2, dW2_ref, 512)] if paired else []):
        for s in range(S):
            _same(tag, "slab %d%s" % (s, name), sl[s * 512 * q:(s + 1) * 512 * q].view(512, q), sl_ref[s])
        _untouched(tag, "the last slab" + name, sl, S * 512 * q)
        _same(tag, "dW" + name, d[:512 * q].view(512, q), d_ref)
        _untouched(tag, "dW" + name, d, 512 * q)
    _report(tag)
    if paired:
        _report(tag + " (second)")


@pytest.mark.parametrize("M", TN_M[64])
def test_weight_gradient_512_is_exact(M):
    _check_wgrad(512, False, M)


@pytest.mark.parametrize("M", TN_M[40])
def test_weight_gradient_768_is_exact(M):
    _check_wgrad(768, False, M)


@pytest.mark.parametrize("M", TN_M[32])
def test_paired_weight_gradient_is_exact(M):
    _check_wgrad(512, True, M)


# ---- kinds 4 and 5: the streaming passes around a dropout ----------------------------------------------------------------------
def _blocks(M):
    """block of each row of a streaming pass (8 rows per block, grid cap 512) and the grid"""
    grid = min(-(-M // 8), 512)
    m = torch.arange(M, device=DEV)
    return (m % (grid * 8)) // 8, grid


@pytest.mark.parametrize("M", STREAM_M)
def test_batchnorm_dropout_pass_is_exact(M):
    e_in, e_out = EXPS[STREAM_M.index(M) % 3]
    tag = "bn_dropout_apply8 M=%d e_in=%d e_out=%d" % (M, e_in, e_out)
    o = _operands()
    keep = _keep()[:M]
    v = o["act"][:M, :512].double() * 2.0 ** e_in
    s, t = o["stats4"][2].double(), o["stats4"][3].double()
    sc, sh = s * 2.0 ** -e_in * 2.0 ** e_out * DP_INV_KEEP, t * 2.0 ** e_out * DP_INV_KEEP
    y = torch.where(keep, v * sc + sh, torch.zeros_like(v))
    _exact_f32(tag, "u", y)
    Cq = e4m3(y)
    if M >= 4095:
        sat = y.abs() > 448
        assert bool(sat.any()) and set(Cq.view(torch.uint8)[sat].tolist()) <= {0x7E, 0xFE}, (tag, "no output beyond 448")
    table = _t({T_IN: e_in, T_OUT: e_out})
    before = table.clone()
    C = _out_rows(M, 512)
    rows = _launch(4, M, table, A=_bytes("act", e_in, 4)[:, :512].contiguous(), bn_stats=o["stats4"], C=C, dp_thresh=DP_THRESH, dp_key=DP_KEY,
                   dp_inv_keep=DP_INV_KEEP)
    assert rows == 0, (tag, rows)
    # the mask on its own, element by element: wherever the kept value is not zero, the stored byte is zero exactly where the hash drops
    shows = (v * sc + sh) != 0
    assert torch.equal(((C[:M] & 0x7F) != 0)[shows], keep[shows]), (tag, "the mask differs from the restated hash")
    _same_bytes(tag, C, M, Cq)
    _table_after(tag, table, before, T_OUT, float(y.abs().max()))
    _report(tag)


@pytest.mark.parametrize("M", STREAM_M)
def test_batchnorm_relu_backward_pass_is_exact(M):
    e_r, e_o = EXPS[STREAM_M.index(M) % 3]
    e_in = e_o - 1
    tag = "bn_relu_bwd8 M=%d e_in=%d e_r=%d e_o=%d" % (M, e_in, e_r, e_o)
    o = _operands()
    gv = o["G"][:M].double()                                                   # as stored
    rv = o["R"][:M, :512].double() * 2.0 ** e_r
    ca, cb, cz = (c.double() for c in o["coef5"])
    inner = (cb * 2.0 ** (e_o - e_r)) * rv + cz * 2.0 ** e_o
    y = torch.where(rv > 0, (ca * 2.0 ** (e_o - e_in)) * gv + inner, torch.zeros_like(gv))
    _exact_f32(tag, "cb r + cz", inner)
    _exact_f32(tag, "y", y)
    Cq = _stored_e5m2(tag, y, M >= 4095)
    assert not bool(Cq.view(torch.uint8)[:, NONPOS].any()), (tag, "column 9 of the reference is not the byte 0")
    block, grid = _blocks(M)
    ref_rows = _worker_sums(tag, "g as stored", Cq.double(), 2.0 ** (e_o - 2), block, grid) * 2.0 ** -e_o
    table = _t({T_IN: e_in, T_R: e_r, T_OUT: e_o})
    before = table.clone()
    G8 = _bytes("G", 0, 5)
    g = G8[:M + GUARD_ROWS].clone()                                            # in place, live gradient rows behind M
    part = _buf(grid * 512)
    rows = _launch(5, M, table, C=g, R=_bytes("R", e_r, 4)[:, :512].contiguous(), coef=o["coef5"], partials=part)
    _same(tag, "output bytes", g[:M], Cq.view(torch.uint8))
    assert torch.equal(g[M:], G8[M:M + GUARD_ROWS]), (tag, "rows behind M were rewritten")
    _table_after(tag, table, before, T_OUT, float(y.abs().max()))
    assert rows == grid, (tag, "partial rows", rows, grid)
    _same_partials(tag, part, rows, 512, ref_rows)
    _report(tag)


# ---- kind 6: the projection's data gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", PROJ_M)
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
def test_projection_data_gradient_is_exact(dropout, M):
    e_r, e_o = EXPS[PROJ_M.index(M) % 3]
    tag = "proj_dgrad8 %s M=%d e_r=%d e_o=%d" % ("p=0.5" if dropout else "no dropout", M, e_r, e_o)
    o = _operands()
    dz, W = o["dz"][:M, :16].double(), o["Wp_t"][:, :16].double()
    _exact_acc(tag, "dz Wp", dz, W.T, 1.0)
    acc = dz @ W.T
    g = torch.where(_keep()[:M], acc * DP_INV_KEEP, torch.zeros_like(acc)) if dropout else acc
    rv = o["R"][:M, :512].double() * 2.0 ** e_r
    ca, cb, cz = (c.double() for c in o["coef6"])
    inner = (cb * 2.0 ** (e_o - e_r)) * rv + cz * 2.0 ** e_o
    y = torch.where(rv > 0, (ca * 2.0 ** e_o) * g + inner, torch.zeros_like(g))
    _exact_f32(tag, "cb r + cz", inner)
    _exact_f32(tag, "y", y)
    Cq = _stored_e5m2(tag, y, M >= 8191)
    assert not bool(Cq.view(torch.uint8)[:, NONPOS].any()), (tag, "column 9 of the reference is not the byte 0")
    worker, n_rows = _workers(M, 32, 256)
    ref_rows = _worker_sums(tag, "C as stored", Cq.double(), 2.0 ** (e_o - 1), worker, 256) * 2.0 ** -e_o
    table = _t({T_R: e_r, T_OUT: e_o})
    before = table.clone()
    C, part = _out_rows(M, 512), _buf(256 * 512)
    drop = dict(dp_thresh=DP_THRESH, dp_key=DP_KEY, dp_inv_keep=DP_INV_KEEP) if dropout else {}
    rows = _launch(6, M, table, A=_bf16("dz"), W=_bf16("Wp_t"), R=_bytes("R", e_r, 4)[:, :512].contiguous(), coef=o["coef6"], C=C, partials=part, **drop)
    if dropout:
        # the mask on its own: where the product and the activation are live, an element is the dropped value cb r + cz exactly where the hash drops
        live = (rv > 0) & (acc != 0)
        dropped = C[:M] == e5m2(torch.where(rv > 0, inner, torch.zeros_like(inner))).view(torch.uint8)
        assert torch.equal(~dropped[live], _keep()[:M][live]), (tag, "the mask differs from the restated hash")
    _same_bytes(tag, C, M, Cq)
    _table_after(tag, table, before, T_OUT, float(y.abs().max()))
    assert rows == n_rows, (tag, "partial rows", rows, n_rows)
    _same_partials(tag, part, rows, 512, ref_rows)
    _report(tag)


# ---- kind 8: the scale table -------------------------------------------------------------------------------------------------------
def fit_exp(amax, target):
    """largest e with amax * 2^e <= target, within -100 .. 100, 0 for amax = 0 (fp8.cuh, f8_fit_exp; tests/test_gpu_fp8.py has it without the clamp)"""
    ma, xa = np.frexp(amax.astype(np.float32))
    mt, xt = np.frexp(np.float32(target))
    e = np.clip(xt - xa - (ma > mt), -100, 100)
    return np.where(amax > 0, e, 0).astype(np.int64)


def ref_update_scales(e, amax_bits, init, n_windows):
    """numpy restatement of fp8_update_scales_kernel"""
    grad = np.arange(F8_NT) >= 16
    e = e.astype(np.int64).copy()
    if not init:
        lg = 0
        while (1 << lg) < 2 * n_windows:
            lg += 1
        e = np.where(grad, lg + 4, 4)
    amax = amax_bits.astype(np.uint32).view(np.float32)
    true = (amax.astype(np.float64) * 2.0 ** (-e.astype(np.float64))).astype(np.float32)
    assert np.array_equal(true.astype(np.float64), amax.astype(np.float64) * 2.0 ** (-e.astype(np.float64))), "the true maximum is not a float32"
    fit = np.where(grad, fit_exp(true, 1024.0), fit_exp(true, 224.0))
    return np.where(amax_bits != 0, fit, e)


@pytest.mark.parametrize("n_windows", [1, 2, 3, 4096, 4097, 167936])
@pytest.mark.parametrize("fresh", [True, False], ids=["fresh", "second_call"])
def test_scale_update_is_exact(fresh, n_windows):
    tag = "fp8_update_scales %s n_windows=%d" % ("fresh" if fresh else "second call", n_windows)
    rng = np.random.default_rng(n_windows)
    e0 = np.zeros(F8_NT, np.int64) if fresh else rng.integers(-12, 20, F8_NT)
    eff = ref_update_scales(e0, np.zeros(F8_NT, np.uint32), not fresh, n_windows)        # the exponents the maxima are read under
    amax = np.zeros(F8_NT, np.float32)
    one_up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    for t in range(F8_NT):
        target = 1024.0 if t >= 16 else 224.0
        at = np.float32(target * 2.0 ** float(eff[t]))                   # stored-unit maximum whose true value is the target
        amax[t] = [0.0, at, one_up(at), at * 2, one_up(at * 2), at / 2, 3.0, 1e-30, 1e30, np.nextafter(at, np.float32(0))][t % 10] if t % 13 else 0.0
    bits = amax.view(np.uint32)
    want_e = ref_update_scales(e0, bits, not fresh, n_windows)
    # a maximum at the target keeps 2^0, one ulp above halves the scale; twice the target likewise one step further
    planted = {1: 0, 2: -1, 3: -1, 4: -2, 5: 1, 9: 0}
    for t in range(F8_NT):
        if t % 13 and t % 10 in planted:
            assert want_e[t] == planted[t % 10], (tag, t, want_e[t])
        if not t % 13 or t % 10 == 0:
            assert want_e[t] == eff[t], (tag, t)
    if fresh:
        lg = {1: 1, 2: 2, 3: 3, 4096: 13, 4097: 14, 167936: 19}[n_windows]
        assert eff[:16].tolist() == [4] * 16 and eff[16:].tolist() == [lg + 4] * 48, (tag, eff)
    table = torch.zeros(256, dtype=torch.int32)
    table[:F8_NT] = torch.from_numpy(e0.astype(np.int32))
    table[F8_NT:2 * F8_NT] = torch.from_numpy(bits.view(np.int32).copy())
    table[128] = 0 if fresh else 1
    table[129:192] = 0x5A5A5A5A
    want = table.clone()
    want[:F8_NT] = torch.from_numpy(want_e.astype(np.int32))
    want[F8_NT:2 * F8_NT] = 0
    want[128] = 1
    table = table.to(DEV)
    rows = _launch(8, n_windows, table)
    assert rows == 0
    got = table.cpu()
    assert torch.equal(got, want), (tag, (got != want).nonzero().flatten().tolist(), got[:F8_NT].tolist(), want[:F8_NT].tolist())


# ---- kind 7: weight preparation --------------------------------------------------------------------------------------------------
def _fit_rows(am):
    return torch.from_numpy(fit_exp(am.float().cpu().numpy(), 448.0)).to(am.device)


@functools.lru_cache(maxsize=None)
def _prep_matrix(rows, cols):
    """integers -7 .. 7 times one power of two per row (2^-3 .. 2^3); planted rows: 0 all zero, 1 with the maximum 56 = 448 2^-3 at
    column 5, 2 the same with one float more, 3 tiny (2^-120: the fitted exponent stops at 100, every entry rounds to zero), 4 huge
    (2^110: the exponent stops at -100, entries pass 448)"""
    gen = torch.Generator(device=DEV).manual_seed(70707 + rows)
    P = torch.randint(-7, 8, (rows, cols), generator=gen, device=DEV).double()
    ex = torch.randint(-3, 4, (rows,), generator=gen, device=DEV).double()
    ex[:5] = torch.tensor([0.0, 0.0, 0.0, -120.0, 110.0], dtype=torch.float64, device=DEV)
    P[0] = 0.0
    P[1, 5] = 56.0
    P[2, 5] = float(np.nextafter(np.float32(56.0), np.float32(100.0)))
    P[3] = P[3].abs()
    P = P * 2.0 ** ex[:, None]
    assert torch.equal(P, P.float().double())
    return P, 2.0 ** ex


@pytest.mark.parametrize("mode,K,ei,eo,affine,t_out", [(0, 512, 0, 0, True, T_OUT), (0, 512, 30, 1, True, T_OUT), (0, 512, -30, -1, False, T_OUT),
                                                        (1, 768, 0, 2, True, T_OUT), (1, 768, -30, 0, True, -1)])
def test_fold_is_exact(mode, K, ei, eo, affine, t_out):
    tag = "fold_linear8 mode=%d K=%d e_in=%d e_out=%d %s t_out=%d" % (mode, K, ei, eo, "affine" if affine else "plain", t_out)
    o = _operands()
    W, rstep = _prep_matrix(512, K)
    k = torch.arange(K, device=DEV)
    ch = k // 12 if mode == 1 else k
    s, t = o["stats4"][2].double().clone(), o["stats4"][3].double().clone()
    s[SAT] = 1.0
    s[ch[5]], t[ch[5]] = 1.0, 0.0                                             # (the planted maxima sit at column 5: they stay the maxima, and the one
                                                                              #  that is no integer adds nothing to the bias)
    b = o["bias"].double()
    if affine:
        w = W * s[ch]
        terms = W * t[ch]
        q = terms.abs().sum(1) / rstep
        assert torch.equal(terms / rstep[:, None], (terms / rstep[:, None]).round()) and float(q.max()) < 2 ** 24, (tag, "W t")
        _note(tag, "sum |W t| / step", q.max())
        acc = terms.sum(1)
    else:
        w, acc = W, torch.zeros(512, dtype=torch.float64, device=DEV)
    _exact_f32(tag, "W s", w)
    am = w.abs().max(1).values
    ej = _fit_rows(am)
    assert ej[:5].tolist() == [0, 3, 2, 100, -100], (tag, ej[:5].tolist())
    q8 = e4m3(w * 2.0 ** ej.double()[:, None]).view(torch.uint8)
    assert not bool(q8[3].any()) and bool((q8[4] & 0x7F == 0x7E).any()), (tag, "the tiny row is not zero or the huge row never clamps")
    kp = (k % 12) * 64 + k // 12 if mode == 1 else k
    want_w = torch.empty_like(q8)
    want_w[:, kp] = q8
    e_out = eo if t_out >= 0 else 0
    sb = (127 + e_out - ej - ei).clamp(1, 254)
    assert (ei == 0) or bool((sb == 1).any()) or bool((sb == 254).any()), (tag, "no scale byte at a clamp")
    want_b = (b + acc).float().double() * 2.0 ** e_out
    _exact_f32(tag, "bias", want_b)
    table = _t({T_IN: ei, T_OUT: eo})
    before = table.clone()
    Wf = W.float().contiguous()
    out_w, out_sc, out_b = _buf(512 * K, torch.uint8), _buf(512, torch.uint8), _buf(512)
    kw = dict(scale=s.float().contiguous(), shift=t.float().contiguous()) if affine else {}
    rows = _launch(7, 512, table, mode=mode, K=K, t_out=t_out, A=Wf, bias=o["bias"], wsc=out_sc, C=out_w, partials=out_b, **kw)
    assert rows == 0, (tag, rows)
    _same(tag, "weight bytes", out_w[:512 * K].view(512, K), want_w)
    _untouched(tag, "the weights", out_w, 512 * K)
    _same(tag, "scale bytes", out_sc[:512], sb.to(torch.uint8))
    _untouched(tag, "the scale bytes", out_sc, 512)
    _same(tag, "bias", out_b[:512], want_b)
    _untouched(tag, "the bias", out_b, 512)
    _table_after(tag, table, before, None, None)
    _report(tag)


@pytest.mark.parametrize("mode,K,eg", [(2, 512, 0), (2, 512, 30), (2, 512, -30), (3, 768, 5)])
def test_weight_transpose_is_exact(mode, K, eg):
    tag = "transpose_w8 mode=%d K=%d e_grad=%d" % (mode, K, eg)
    P, _ = _prep_matrix(K, 512)                                               # row k of P = column k of W
    ek = _fit_rows(P.abs().max(1).values)
    assert ek[:5].tolist() == [0, 3, 2, 100, -100], (tag, ek[:5].tolist())
    q8 = e4m3(P * 2.0 ** ek.double()[:, None]).view(torch.uint8)
    kp = torch.arange(K, device=DEV)
    k = (kp & 63) * 12 + (kp >> 6) if mode == 3 else kp                       # row kp of the output = column k of W
    sb = (127 - ek - eg).clamp(1, 254)
    assert eg == 0 or mode == 3 or bool((sb == 1).any()) or bool((sb == 254).any()), (tag, "no scale byte at a clamp")
    table = _t({T_IN: eg})
    before = table.clone()
    W = P.T.float().contiguous()
    out_w, out_sc = _buf(K * 512, torch.uint8), _buf(K, torch.uint8)
    rows = _launch(7, 512, table, mode=mode, K=K, A=W, wsc=out_sc, C=out_w)
    assert rows == 0, (tag, rows)
    _same(tag, "weight bytes", out_w[:K * 512].view(K, 512), q8[k])
    _untouched(tag, "the weights", out_w, K * 512)
    _same(tag, "scale bytes", out_sc[:K], sb[k].to(torch.uint8))
    _untouched(tag, "the scale bytes", out_sc, K)
    _table_after(tag, table, before, None, None)
    _report(tag)
