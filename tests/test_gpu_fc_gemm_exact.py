"""The large-batch fc GEMM kernels on their own, one launch at a time through cp_debug_fc_gemm, at tolerance ZERO.

Which launch reaches which kernel (csrc/encoder_api.cuh launch_fc_gemm; bf16):

    launch                                   CP_TILES_STATIC                     CP_TILES_DYNAMIC
    forward, K = 512                         gemm_ws16                           gemm_nt256p<EPI_FWD, dyn>
    forward, K = 768 (fc1)                   gemm_ws16n                          gemm_nt256p<EPI_FWD, dyn>
    data gradient, no saved activation       gemm_nt256p<EPI_DGRAD, static>      gemm_nt256p<EPI_DGRAD, dyn>
    data gradient, R and coef (BN mode)      gemm_wsd16<0>                       gemm_nt256p<EPI_DGRAD_BN, dyn>
    data gradient, R, no coef (ST mode)      gemm_wsd16<1>                       gemm_nt256p<EPI_DGRAD_ST, dyn>   (with and without dropout)
    weight gradient                          gemm_tn256                          gemm_tn256
    K = 64 (the projection's data gradient): every launch above with R runs the persistent kernel under BOTH schedules, on one K
    block -- <EPI_DGRAD_BN | EPI_DGRAD_ST, static> where K = 512 reaches gemm_wsd16

Why zero: the operands are ternary (-1 / 1 with probability 1/16 each, else 0), the bias, the saved activation and the BatchNorm
coefficients small integers or halves.  Every product is then -1, 0 or 1, every float32 accumulator an integer far below 2^24
whatever the order of its additions, every value the kernels round to bf16 is a bf16 number already, and every column sum is a
sum of such numbers below 2^24 steps: a launch has ONE right answer, bit for bit, whichever block ran which tile and however the
sums were grouped.  The reference is the same operation in float64 torch.  The test asserts these preconditions on its reference
before it compares anything (`_exact_stat`, `_exact_values`), so a changed recipe cannot quietly make it approximate.

What is compared (torch.equal): every element of C in rows < M; the guard rows behind M still hold the sentinel bit pattern the
buffer was filled with (a NaN: the data cannot produce it); the `stat_rows_out` partial rows summed in float64 against the
reference column sums; under the dynamic schedule partial row t against the sums of sample tile t alone (rows 256t .. 256t + 255:
what bn_finalize and the reproducibility claim rest on); the floats behind the last partial row are untouched; the weight
gradient's slabs summed over S against X^T Y.  Dropout (p = 0.5: threshold 32768, 1 / (1 - p) = 2 exactly): every output is 0 or
twice the undropped reference, the zero pattern is the same under both schedules, the kept share lies within 6 binomial standard
deviations of 0.5, and -- the numpy restatement of the hash in tools/dropout_hash_check.py can be driven with dropout_pair's
(key, row, ld, column): quad index (row * ld + column) >> 2, draw column & 3 -- the mask equals that restatement element by element.

Shapes: every model shape of the launch kind, M in rows (the entry has no 41-window groups): 1 (one live row, clamped source rows,
seven XCDs without an item), 255 / 256 / 257 (the tile boundary), 2,049 (nine sample tiles, XCD 0's second holds one live row),
32,801 at F = 512 and 20,513 at F = 768 (129 / 81 sample tiles ragged by 33 rows: a block takes a second tile), 45,057 at F = 768
(177 sample tiles, 69 items on XCD 0's 32 blocks: a third tile, the s_item slots wrap; three rounds of the static assignment);
and, for the kernels only the static schedule reaches, a multiple of the kernel's row tile times its workers plus one tile, one
row more and one row less (WS16_RT = WSN_RT = 48, WSD16_RT = 32; the weight gradient: the rounding of its rows per split).
K = 64, F = 512 (the 64 columns of dz against the projection's transposed weight; all 64 columns live here): the same M table.

Each case prints the largest |value| and the largest column sum of |values| in steps it saw (pytest -s): the margin to 2^24."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATIC, DYNAMIC = 0, 1
SCHEDULES = ((STATIC, "static"), (DYNAMIC, "dynamic"))
M_MAX = 45057
GUARD_ROWS = 320                        # more than one 256-row tile: a ragged tile stored whole would land here
C_SENTINEL = 0x7FA5                     # a bf16 NaN
P_SENTINEL = 0x7FC0BEEF                 # a float32 NaN
P_FLOATS = 256 * 2 * 768 + 8192         # more partial rows than any launch here writes (177 sample tiles, 128 workers) + guard
DP_THRESH, DP_INV_KEEP, DP_KEY = 32768, 2.0, 0x5EED1234           # p = 0.5: round(p * 65536), 1 / (1 - 32768 / 65536)

TABLE_512 = [1, 255, 256, 257, 2049, 32801]
TABLE_768 = [1, 255, 256, 257, 2049, 20513, 45057]
# one tile more than a full round of the static kernel's workers, and a row either side of it
WS16_M = [48 * 129 - 1, 48 * 129, 48 * 129 + 1]                  # gemm_ws16, F = 512: 16 workers x 8 XCDs, 48-row tiles
WSN_M = [48 * 65 - 1, 48 * 65, 48 * 65 + 1]                      # gemm_ws16n, F = 512: 8 workers x 8 XCDs, 48-row tiles
WSD512_M = [32 * 129 - 1, 32 * 129, 32 * 129 + 1]                # gemm_wsd16, F = 512: 16 workers x 8 XCDs, 32-row tiles
WSD768_M = [32 * 81 - 1, 32 * 81, 32 * 81 + 1]                   # gemm_wsd16, F = 768: 10 workers x 8 XCDs
TN512_M = [1, 2047, 2048, 2049, 32801]                           # 64 splits of 32 rows: 2,049 rows round up to 33 splits of 64
TN768_M = [1, 1279, 1280, 1281, 20513]                           # 40 splits


def _ternary(shape, gen):
    u = torch.randint(0, 16, shape, generator=gen, device="cuda")
    return ((u == 0).float() - (u == 1).float()).bfloat16()


@functools.lru_cache(maxsize=None)
def _operands(K, F):
    """the recipe of the module docstring, made once per shape: slices [:M] serve every case (rows behind M hold live data: a
    kernel that read them would show it in the sums)"""
    gen = torch.Generator(device="cuda").manual_seed(1000 * K + F)
    A = _ternary((M_MAX, K), gen)
    W = _ternary((F, K), gen)
    Y = _ternary((M_MAX, F), gen)                                                     # the weight gradient's second operand
    bias = torch.randint(-3, 4, (F,), generator=gen, device="cuda").float()
    R = torch.relu(torch.randint(-2, 4, (M_MAX, F), generator=gen, device="cuda").float()).bfloat16()
    return dict(A=A, W=W, Y=Y, bias=bias, R=R)


@functools.lru_cache(maxsize=None)
def _coef(mod):
    gen = torch.Generator(device="cuda").manual_seed(77 + mod)
    ca = torch.tensor([0.5, 1.0, 2.0], device="cuda")[torch.randint(0, 3, (mod,), generator=gen, device="cuda")]
    cb = torch.randint(-1, 2, (mod,), generator=gen, device="cuda").float()
    cz = torch.randint(-2, 3, (mod,), generator=gen, device="cuda").float()
    # [3][coef_mod] at the front of a larger buffer of NaN: an entry read with the wrong modulus lands in bounds and shows
    room = torch.full((4096,), float("nan"), device="cuda")
    room[:3 * mod] = torch.stack([ca, cb, cz]).flatten()
    return room[:3 * mod].view(3, mod)


def _c_buffer(M, F):
    c = torch.empty(M + GUARD_ROWS, F, dtype=torch.bfloat16, device="cuda")
    c.view(torch.int16).fill_(C_SENTINEL)
    return c


def _p_buffer(n=P_FLOATS):
    p = torch.empty(n, dtype=torch.float32, device="cuda")
    p.view(torch.int32).fill_(P_SENTINEL)
    return p


def _launch(kind, schedule, M, K, F, A, W, C, bias=None, R=None, partials=None, coef=None, coef_mod=0, dropout=False, stream=None):
    from contrastiveprosthetics_amd import _lib
    d = _lib.cp_debug_fc_gemm_args()
    d.dtype, d.kind, d.M, d.K, d.F, d.tile_schedule, d.coef_mod = _lib.CP_BF16, kind, M, K, F, schedule, coef_mod
    d.A, d.W, d.C = A.data_ptr(), W.data_ptr(), C.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.R = R.data_ptr() if R is not None else None
    d.partials = partials.data_ptr() if partials is not None else None
    d.coef = coef.data_ptr() if coef is not None else None
    if dropout:
        d.dp_thresh, d.dp_key, d.dp_inv_keep = DP_THRESH, DP_KEY, DP_INV_KEEP
    rows = ctypes.c_int32(-1)
    d.stat_rows_out = ctypes.pointer(rows)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    _lib.check(_lib.load().cp_debug_fc_gemm(ctypes.byref(d), st), "cp_debug_fc_gemm")
    return rows.value


# ---- the preconditions of "tolerance zero", asserted on the reference ------------------------------------------------------
SEEN = {}


def _exact_values(tag, ref):
    """the values a kernel rounds to bf16 are bf16 numbers already"""
    assert torch.equal(ref, ref.bfloat16().double()), tag
    SEEN.setdefault(tag, {})["max |value|"] = float(ref.abs().max())


def _exact_stat(tag, name, terms, step):
    """a column sum of `terms` is exact in float32 in any order and grouping: every term is an integer multiple of `step`, and even the
    column sums of |term| stay below 2^24 steps"""
    q = terms / step
    assert torch.equal(q, q.round()), (tag, name)
    top = float(q.abs().sum(0).max())
    assert top < 2 ** 24, (tag, name, top)
    SEEN.setdefault(tag, {})["sum |%s| / step" % name] = top


def _report(tag):
    print("\n[fc_gemm_exact] %s: %s (2^24 = 16777216)" % (tag, ", ".join("%s %g" % kv for kv in SEEN.get(tag, {}).items())))


# ---- comparisons ----------------------------------------------------------------------------------------------------------------
def _where(got, ref):
    """which rows, column tiles and XCD residues (row / 256 % 8) differ: informative by construction of the schedules"""
    bad = got != ref                                            # (a sentinel NaN left in place differs from everything)
    rows = bad.any(1).nonzero().flatten()
    cols = bad.any(0).nonzero().flatten()
    return "%d elements differ; rows %s .. %s (%d rows), sample tiles %s, XCD residues %s, column tiles %s, first columns %s" % (
        int(bad.sum()), rows[:8].tolist(), rows[-3:].tolist(), rows.numel(), torch.unique(rows // 256)[:12].tolist(),
        torch.unique(rows // 256 % 8).tolist(), torch.unique(cols // 256).tolist(), cols[:8].tolist())


def _check_c(tag, C, M, ref):
    guard = C[M:].view(torch.int16)
    assert torch.equal(guard, torch.full_like(guard, C_SENTINEL)), (tag, "rows behind M were written")
    got = C[:M].double()
    assert torch.equal(got, ref), (tag, _where(got, ref))


def _tile_sums(terms):
    """[tiles][F]: the column sums of each 256-row sample tile"""
    M, F = terms.shape
    tiles = (M + 255) // 256
    pad = torch.zeros(tiles * 256, F, dtype=terms.dtype, device=terms.device)
    pad[:M] = terms
    return pad.view(tiles, 256, F).sum(1)


def _check_partials(tag, P, n, n_expected, stats, dynamic):
    """stats: the launch's statistics in the order of its partial rows ([n][len(stats)][F]), each the [M][F] terms it sums"""
    assert n == n_expected, (tag, "partial rows", n, n_expected)
    F = stats[0].shape[1] if stats else 0
    width = len(stats) * F
    tail = P[n * width:].view(torch.int32)
    assert torch.equal(tail, torch.full_like(tail, P_SENTINEL)), (tag, "floats behind the last partial row were written")
    if not stats:
        return
    body = P[:n * width].view(n, len(stats), F).double()
    for i, terms in enumerate(stats):
        got, ref = body[:, i].sum(0), terms.sum(0)
        assert torch.equal(got, ref), (tag, "column sums of statistic %d" % i, (got != ref).nonzero().flatten()[:8].tolist())
        if dynamic:
            per_tile = _tile_sums(terms)
            assert torch.equal(body[:, i], per_tile), (tag, "statistic %d per sample tile" % i, _where(body[:, i], per_tile))


def _tiles(M, rt=256):
    return (M + rt - 1) // rt


# ---- forward -------------------------------------------------------------------------------------------------------------------
def _forward_reference(tag, K, F, M):
    o = _operands(K, F)
    ref = torch.relu(o["A"][:M].double() @ o["W"].double().T + o["bias"].double())
    _exact_values(tag, ref)
    _exact_stat(tag, "v", ref, 1.0)
    _exact_stat(tag, "v^2", ref * ref, 1.0)
    return o, ref


@pytest.mark.parametrize("K,F,M", [(768, 512, m) for m in TABLE_512 + WSN_M] + [(512, 512, m) for m in TABLE_512 + WS16_M])
def test_forward_is_exact(K, F, M):
    tag = "forward K=%d F=%d M=%d" % (K, F, M)
    o, ref = _forward_reference(tag, K, F, M)
    workers = 128 if K == 512 else 64                                  # gemm_ws16: 32 / (F / 256) x 8; gemm_ws16n: 32 / (F / 128) x 8
    for schedule, name in SCHEDULES:
        C, P = _c_buffer(M, F), _p_buffer()
        n = _launch(0, schedule, M, K, F, o["A"], o["W"], C, bias=o["bias"], partials=P)
        torch.cuda.synchronize()
        _check_c(tag + " " + name, C, M, ref)
        _check_partials(tag + " " + name, P, n, _tiles(M) if schedule else min(_tiles(M, 48), workers), [ref, ref * ref], schedule == DYNAMIC)
    _report(tag)


# ---- data gradient without a saved activation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,F,M", [(512, 512, m) for m in TABLE_512] + [(512, 768, m) for m in TABLE_768] + [(64, 512, m) for m in TABLE_512])
def test_plain_data_gradient_is_exact(K, F, M):
    o = _operands(K, F)
    tag = "dgrad K=%d F=%d M=%d" % (K, F, M)
    ref = o["A"][:M].double() @ o["W"].double().T
    _exact_values(tag, ref)
    for schedule, name in SCHEDULES:
        C, P = _c_buffer(M, F), _p_buffer()
        n = _launch(1, schedule, M, K, F, o["A"], o["W"], C, partials=P)
        torch.cuda.synchronize()
        _check_c(tag + " " + name, C, M, ref)
        _check_partials(tag + " " + name, P, n, 0, [], schedule == DYNAMIC)             # no sums: nothing is written
    _report(tag)


# ---- data gradient with BatchNorm + ReLU backward of the layer below in the epilogue ----------------------------------------------
def _bn_reference(tag, K, F, mod, M):
    o, coef = _operands(K, F), _coef(mod)
    acc = o["A"][:M].double() @ o["W"].double().T
    r = o["R"][:M].double()
    ca, cb, cz = (coef[i].double()[torch.arange(F, device="cuda") % mod] for i in range(3))
    ref = torch.where(r > 0, ca * acc + cb * r + cz, torch.zeros_like(acc))
    _exact_values(tag, ref)
    _exact_stat(tag, "g", ref, 0.5)
    return o, coef, ref


def _static_rows(K, F, M):
    """partial rows of a data gradient with R under the static schedule: gemm_wsd16 (K = 512) writes one per worker that drew a 32-row
    tile, the persistent kernel (any other K) one per slot of a round of 256-row sample tiles: 32 / (F / 256) x 8 either way"""
    workers = (32 // (F // 256)) * 8
    return min(_tiles(M, 32 if K == 512 else 256), workers)


@pytest.mark.parametrize("K,F,mod,M", [(512, 512, 512, m) for m in TABLE_512 + WSD512_M] + [(512, 768, 64, m) for m in TABLE_768 + WSD768_M] +
                         [(64, 512, 512, m) for m in TABLE_512])
def test_bn_mode_data_gradient_is_exact(K, F, mod, M):
    """F = 768 with coef_mod = 64: fc1's gradient into the conv layout, where feature f takes channel f % 64's coefficients.
    K = 64 with coef_mod = 512: the projection's data gradient without a dropout in front of it"""
    tag = "dgrad+BN K=%d F=%d coef_mod=%d M=%d" % (K, F, mod, M)
    o, coef, ref = _bn_reference(tag, K, F, mod, M)
    for schedule, name in SCHEDULES:
        C, P = _c_buffer(M, F), _p_buffer()
        n = _launch(1, schedule, M, K, F, o["A"], o["W"], C, R=o["R"], partials=P, coef=coef, coef_mod=mod)
        torch.cuda.synchronize()
        _check_c(tag + " " + name, C, M, ref)
        _check_partials(tag + " " + name, P, n, _tiles(M) if schedule else _static_rows(K, F, M), [ref], schedule == DYNAMIC)
    _report(tag)


# ---- data gradient behind a dropout: the mask and the two BatchNorm-backward sums ---------------------------------------------------
def _hash_keep(M, F):
    """the kernels' keep decision for element (m, f) of an [M][F] tensor, from the numpy restatement of csrc/common.cuh dropout_quad"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dropout_hash_check as dh
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(F // 4) + np.arange(F // 4, dtype=np.uint64)[None, :]
    a, b = dh.quad(idx, np.uint64(DP_KEY))
    draws = np.stack(dh.draws(a, b), axis=-1).reshape(M, F)              # quad (m * F + f) >> 2, draw f & 3
    return torch.from_numpy(draws >= DP_THRESH).cuda()


@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("M", TABLE_512 + WSD512_M)
def test_st_mode_data_gradient_is_exact(M, dropout):
    _st_mode_case(512, M, dropout)


@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("M", TABLE_512)
def test_st_mode_data_gradient_of_the_projection_is_exact(M, dropout):
    """K = 64: the projection's data gradient on the unfused route, with and without the dropout behind fc7"""
    _st_mode_case(64, M, dropout)


def _st_mode_case(K, M, dropout):
    F = 512
    o = _operands(K, F)
    tag = "dgrad+ST K=%d F=%d M=%d %s" % (K, F, M, "p=0.5" if dropout else "no dropout")
    acc = o["A"][:M].double() @ o["W"].double().T
    r = o["R"][:M].double()
    keep = _hash_keep(M, F) if dropout else torch.ones_like(acc, dtype=torch.bool)
    ref = torch.where(keep, acc * (DP_INV_KEEP if dropout else 1.0), torch.zeros_like(acc))
    _exact_values(tag, ref)
    _exact_stat(tag, "g", ref, 1.0)
    _exact_stat(tag, "g r", ref * r, 1.0)
    got = {}
    for schedule, name in SCHEDULES:
        C, P = _c_buffer(M, F), _p_buffer()
        n = _launch(1, schedule, M, K, F, o["A"], o["W"], C, R=o["R"], partials=P, dropout=dropout)
        torch.cuda.synchronize()
        got[schedule] = C[:M].double()
        if dropout:
            # what holds without knowing the hash: 0 or twice the undropped product, kept about half the time
            c, live = got[schedule], acc != 0
            assert bool(((c == 0) | (c == 2 * acc)).all()), (tag, name, "an output is neither 0 nor twice the undropped reference")
            count = int(live.sum())
            share = float(((c != 0) & live).sum()) / count
            assert abs(share - 0.5) <= 6 * (0.25 / count) ** 0.5, (tag, name, share, count)
        _check_c(tag + " " + name, C, M, ref)                                              # ... and the mask is the hash's
        _check_partials(tag + " " + name, P, n, _tiles(M) if schedule else _static_rows(K, F, M), [ref, ref * r], schedule == DYNAMIC)
    live = acc != 0
    assert torch.equal((got[STATIC] == 0) & live, (got[DYNAMIC] == 0) & live), (tag, "the schedules drop different elements")
    _report(tag)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P_,Q,M", [(512, 512, m) for m in TN512_M] + [(512, 768, m) for m in TN768_M])
def test_weight_gradient_slabs_sum_to_the_product(P_, Q, M):
    """slabs[S][P][Q] summed over S = X^T Y.  S is the host layer's: rows per split = M / (64 | 40) rounded up to 32 rows."""
    o = _operands(P_, Q)
    tag = "wgrad P=%d Q=%d M=%d" % (P_, Q, M)
    X, Y = o["A"][:M].double(), o["Y"][:M].double()
    ref = X.T @ Y
    _exact_stat(tag, "x y", (X.abs().T @ Y.abs()).unsqueeze(0), 1.0)                  # column sums of |x y| per entry
    assert torch.equal(ref, ref.round())
    target = 64 if Q == 512 else 40
    per_split = -(-M // target)
    rps = -(-per_split // 32) * 32
    S_expected = -(-M // rps)
    for schedule, name in SCHEDULES:                                          # (one kernel: the schedule must not matter)
        slabs = _p_buffer((target + 1) * P_ * Q + 8192)
        S = _launch(2, schedule, M, P_, Q, o["A"], o["Y"], slabs)
        torch.cuda.synchronize()
        assert S == S_expected, (tag, name, S, S_expected)
        tail = slabs[S * P_ * Q:].view(torch.int32)
        assert torch.equal(tail, torch.full_like(tail, P_SENTINEL)), (tag, name, "floats behind the last slab were written")
        got = slabs[:S * P_ * Q].view(S, P_, Q).double().sum(0)
        assert torch.equal(got, ref), (tag, name, _where(got, ref))
    _report(tag)


# ---- the tile counters and the per-stream counter slots (dynamic schedule) -------------------------------------------------------
def _bn_case(M):
    return _bn_reference("counters BN M=%d" % M, 512, 768, 64, M)


def _fwd_case(M):
    return _forward_reference("counters forward M=%d" % M, 512, 512, M)


def test_back_to_back_launches_find_their_counters_at_zero():
    """two launches on one stream, nothing between them, another M for the second: the last block of the first must have left the
    XCD counters and the blocks-finished count at zero, or the second draws no tiles and its C keeps the sentinel.  A plain sequence,
    run once: forward then forward, BN-mode gradient then BN-mode gradient."""
    M1, M2 = 2049, 257
    o, ref1 = _fwd_case(M1)
    _, ref2 = _fwd_case(M2)
    C1, P1, C2, P2 = _c_buffer(M1, 512), _p_buffer(), _c_buffer(M2, 512), _p_buffer()
    torch.cuda.synchronize()
    n1 = _launch(0, DYNAMIC, M1, 512, 512, o["A"], o["W"], C1, bias=o["bias"], partials=P1)
    n2 = _launch(0, DYNAMIC, M2, 512, 512, o["A"], o["W"], C2, bias=o["bias"], partials=P2)
    torch.cuda.synchronize()
    _check_c("first forward", C1, M1, ref1)
    _check_partials("first forward", P1, n1, _tiles(M1), [ref1, ref1 * ref1], True)
    _check_c("second forward", C2, M2, ref2)
    _check_partials("second forward", P2, n2, _tiles(M2), [ref2, ref2 * ref2], True)

    o, coef, ref1 = _bn_case(M1)
    _, _, ref2 = _bn_case(M2)
    C1, P1, C2, P2 = _c_buffer(M1, 768), _p_buffer(), _c_buffer(M2, 768), _p_buffer()
    torch.cuda.synchronize()
    n1 = _launch(1, DYNAMIC, M1, 512, 768, o["A"], o["W"], C1, R=o["R"], partials=P1, coef=coef, coef_mod=64)
    n2 = _launch(1, DYNAMIC, M2, 512, 768, o["A"], o["W"], C2, R=o["R"], partials=P2, coef=coef, coef_mod=64)
    torch.cuda.synchronize()
    _check_c("first BN gradient", C1, M1, ref1)
    _check_partials("first BN gradient", P1, n1, _tiles(M1), [ref1], True)
    _check_c("second BN gradient", C2, M2, ref2)
    _check_partials("second BN gradient", P2, n2, _tiles(M2), [ref2], True)


def test_a_second_stream_draws_from_its_own_counters():
    """the same launch on a second stream (its own counter slot) while the first stream's result is still to be read: both exact"""
    M = 2049
    o, ref = _fwd_case(M)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = [(_c_buffer(M, 512), _p_buffer()) for _ in range(2)]
    torch.cuda.synchronize()                                                # operands and sentinels are in place for both streams
    rows = [_launch(0, DYNAMIC, M, 512, 512, o["A"], o["W"], C, bias=o["bias"], partials=P, stream=s) for (C, P), s in zip(bufs, (s1, s2))]
    s1.synchronize()
    s2.synchronize()
    for (C, P), n, name in zip(bufs, rows, ("first stream", "second stream")):
        _check_c(name, C, M, ref)
        _check_partials(name, P, n, _tiles(M), [ref, ref * ref], True)
