"""The large-batch conv launches on their own, one at a time through cp_debug_conv, at tolerance ZERO and ragged window counts.

Which kind launches which kernels (csrc/api.hip debug_conv_t, through the launch functions of the step in csrc/encoder_api.cuh):

    kind  launches                                                               what is read back
    0     conv1_stats_kernel<T>                                                  partial rows [g][2][64] (sum, sum of squares of r1), g
    1     prep_conv2_kernel<T>, conv2_strip_kernel<T, 0>                         out [N*12][64] T, partial rows [grid][2][64], grid
    2     prep_conv2_kernel<T>, conv2_strip_kernel<T, 1>                         the data gradient [N*12][64] T, partial rows [grid][2][64]
    3     (colsum_kernel<T>,) conv2_wgrad_kernel<T> | <T, true>,                 slabs [S][64][192], the 32 folded slabs, dW2, rows2 [64][2][64], S
          reduce_rows_kernel (S > 64), conv2_wgrad_finish_kernel<T>
    4     prep_conv2_kernel<T>, conv2_dgrad_conv1_kernel<T> | <T, true>,         partial rows [grid][4][64], the 32 folded rows, dW1, db1, grid
          reduce_rows_kernel (grid > 64), conv1_bwd_finalize_kernel

These are the non-small template branches, at every N -- also below the 2,625 windows from which the step dispatches them.

Why zero: x, the conv taps, the biases and the gradient are -1 / 0 / 1 (the gradient with density 1/8, conv2's weights with 6
non-zeros per output channel), BatchNorm1's scale is 1 or 2 and its shift -1 / 0 / 1, the backward coefficients are halves and small
integers.  Then r1 is in 0..4, u1 in -1..9, conv2's output at most 6 * 9 + 3 = 57, the data gradient at most 192, ca g + cb r1 + cz a
multiple of 0.5 below 2^10: every value a kernel rounds to T is a T number already, and every f32 accumulator is an integer (or a
multiple of 0.5) far below 2^24 steps whatever the order of its additions.  A launch has ONE right answer, bit for bit, whichever
block ran which strip.  The preconditions are asserted on the float64 reference before anything is compared (`_exact_values`,
`_exact_stat`), so a changed recipe cannot quietly make the test approximate.  Kernel rows 0 and 2 of both convolutions hold
sentinels (7 and 5) that would show if read; rows 0 and 1 of stats1 are NaN; rows of x and of the gradient behind N hold live data.

The reference is float64 torch, written from the operation: conv1 = 3-tap correlation over 12 zero-padded positions + ReLU; conv2 =
the same over u1 = s r1 + t, zero-padded AFTER the affine map; the data gradient = the transposed correlation; the raw product
P[o][tap][c] = sum g[n][q][o] r1[n][q + tap - 1][c]; dW2 = the correlation of g with the padded u1 (= s P + t G); rows2[o] = (sum_tap
W2[o][c][tap] G[o][tap], sum_tap W2[o][c][tap] P[o][tap][c]); conv1's gradients from gy = [r1 > 0] (ca g_v1 + cb r1 + cz).

Compared with torch.equal: every output row below N * 12; the guard rows behind (320: more than one 192-row strip) still hold the NaN
sentinel; the floats behind the reported partial rows, slabs, folded slabs and folded rows likewise; partial row b = the reference
sums over exactly the strips b, b + grid, b + 2 grid, .. (the assignment is static: a block that took a wrong strip shows), slab b
= the raw product of strips b, b + S, ..; folded slab / row s = the sum of slabs / rows s, s + 32, ..; their totals = the
whole-tensor reference; dW2 / dW1 kernel rows 0 and 2 exactly zero; rows2, db1; g, grid, S and the column-sum rows against the host
arithmetic restated in `host_plan`, itself pinned by this table:

    strip kernels (kinds 1, 2, 4; 16 windows per strip; grid = min(strips, 512 | f32 256); pre-reduce above 64 rows)
        N      1   15   16   17   1024   1025   4096   4097   8192   8193   8245
        bf16   1    1    1    2     64     65    256    257    512    512    512      (8,193: block 0's second strip holds one window)
        f32    1    1    1    2     64     65    256    256
    weight gradient (kind 3; 8 windows per strip; S = min(strips, 512 | f32 256); the slab fold above 64 slabs)
        N      1    7    8    9    512    513   2048   2049   4096   4097
        bf16   1    1    1    2     64     65    256    257    512    512
        f32    1    1    1    2     64     65    256    256
      colsum_kernel rows = min(ceil(N / 2), 256) in bf16, min(N, 256) in f32: a second pass from 513 | 257 windows on
    conv1 statistics (kind 0; 32 | f32 16 windows per block and pass, 2,048 blocks per pass, every block the same number of passes)
        bf16   N   1   31   32   33   65,536   65,537        f32   N   15   16   17   32,768   32,769
               g   1    1    1    2    2,048    1,025              g    1    1    2    2,048    1,025

Kind 3 runs each shape with colsum_kernel making the column sums and with caller rows, nr = 1, 21, 22, 300 (the finish kernel walks
them in 21 lanes).  The e5m2 forms (<T, true>) read the bytes of {-1, 0, 1} * 2^e with gin_exp = e, e = 0 and 3, at N = 1, 17 and
4,097 (kind 3) | 8,193 (kind 4).  Kinds 1 and 2 run twice, the out buffer pre-filled with NaN and with 1.0: no read-modify-write.

Each case prints the largest |value| and the largest column sum of |values| in steps it saw (pytest -s): the margin to 2^24."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda" if torch.cuda.is_available() else "cpu"        # (the reference alone also runs on a CPU: the preconditions were confirmed there)
BF16, F32 = 1, 0
TORCH_T = {BF16: torch.bfloat16, F32: torch.float32}
NAME_T = {BF16: "bf16", F32: "f32"}
NX = 65537 + 64                         # windows of x: live data behind every N
NG = 8245 + 32                          # windows of the gradient
GUARD_ROWS = 320                        # more than one 192-row strip
SENT16, SENT32 = 0x7FA5, 0x7FC0BEEF     # a bf16 NaN, a float32 NaN
P_FLOATS = 2048 * 128 + 8192            # more partial rows than any launch here writes (conv1: 2,048 rows of 128) + guard
SLAB = 64 * 192
W2_NNZ = 6                              # (12 put the sum of squares of conv2's output past 2^24 at 8,192 windows: 17,678,391)
NAN = float("nan")

STRIP_N = {BF16: [1, 15, 16, 17, 1024, 1025, 8192, 8193, 8245], F32: [1, 15, 16, 17, 1024, 1025, 4096, 4097]}
WGRAD_N = {BF16: [1, 7, 8, 9, 512, 513, 4096, 4097], F32: [1, 7, 8, 9, 512, 513, 2048, 2049]}
CONV1_N = {BF16: [1, 31, 32, 33, 65536, 65537], F32: [15, 16, 17, 32768, 32769]}
GCOL_NR = [1, 21, 22, 300]


def _cases(table):
    return [pytest.param(dt, n, id="%s-%d" % (NAME_T[dt], n)) for dt in (BF16, F32) for n in table[dt]]


# ---- the host arithmetic, restated (csrc/encoder_api.cuh: conv_grid, conv2_wgrad, launch_conv2_gcols, launch_conv1_stats) ------------
def host_plan(dtype, N):
    cap = 512 if dtype == BF16 else 256
    cdiv = lambda a, b: -(-a // b)
    rpp = 32 if dtype == BF16 else 16
    need = cdiv(N, rpp)
    passes = cdiv(need, 2048)
    return dict(grid=min(cdiv(N, 16), cap), S=min(cdiv(N, 8), cap), gcol_rows=min(cdiv(N, 2 if dtype == BF16 else 1), 256),
                g=cdiv(need, passes), conv1_rpp=rpp)


def test_host_plan_matches_the_table():
    strip = {BF16: dict(zip([1, 15, 16, 17, 1024, 1025, 4096, 4097, 8192, 8193, 8245], [1, 1, 1, 2, 64, 65, 256, 257, 512, 512, 512])),
             F32: dict(zip([1, 15, 16, 17, 1024, 1025, 4096, 4097], [1, 1, 1, 2, 64, 65, 256, 256]))}
    wg = {BF16: dict(zip([1, 7, 8, 9, 512, 513, 2048, 2049, 4096, 4097], [1, 1, 1, 2, 64, 65, 256, 257, 512, 512])),
          F32: dict(zip([1, 7, 8, 9, 512, 513, 2048, 2049], [1, 1, 1, 2, 64, 65, 256, 256]))}
    c1 = {BF16: dict(zip([1, 31, 32, 33, 65536, 65537], [1, 1, 1, 2, 2048, 1025])),
          F32: dict(zip([15, 16, 17, 32768, 32769], [1, 1, 2, 2048, 1025]))}
    for dt in (BF16, F32):
        for n, v in strip[dt].items():
            assert host_plan(dt, n)["grid"] == v, (dt, n)
        for n, v in wg[dt].items():
            assert host_plan(dt, n)["S"] == v, (dt, n)
        for n, v in c1[dt].items():
            assert host_plan(dt, n)["g"] == v, (dt, n)
        assert all(n in strip[dt] for n in STRIP_N[dt]) and all(n in wg[dt] for n in WGRAD_N[dt]) and all(n in c1[dt] for n in CONV1_N[dt])
    assert [host_plan(BF16, n)["gcol_rows"] for n in (1, 7, 8, 9, 512, 513)] == [1, 4, 4, 5, 256, 256]
    assert [host_plan(F32, n)["gcol_rows"] for n in (1, 9, 256, 257, 513)] == [1, 9, 256, 256, 256]


# ---- the recipe ----------------------------------------------------------------------------------------------------------------
class _Inputs:
    pass


@functools.lru_cache(maxsize=None)
def _inputs():
    """made once on the host generator (the same numbers on every device), float32; rows behind any N hold live data"""
    gen = torch.Generator().manual_seed(20261019)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=gen)
    I = _Inputs()
    I.x = ri(-1, 2, (NX, 12)).float()
    I.w1 = torch.full((64, 1, 3, 3), 7.0)
    I.w1[:, :, 1, :] = ri(-1, 2, (64, 1, 3)).float()
    I.b1 = ri(-1, 2, (64,)).float()
    I.stats1 = torch.full((4, 64), NAN)
    I.stats1[2] = ri(1, 3, (64,)).float()
    I.stats1[3] = ri(-1, 2, (64,)).float()
    I.w2 = torch.full((64, 64, 3, 3), 5.0)
    taps = torch.zeros(64, 192)
    for o in range(64):                                    # W2_NNZ non-zeros among the 64 x 3 taps of an output channel
        taps[o, torch.randperm(192, generator=gen)[:W2_NNZ]] = (ri(0, 2, (W2_NNZ,)) * 2 - 1).float()
    I.w2[:, :, 1, :] = taps.view(64, 64, 3)
    I.b2 = ri(-3, 4, (64,)).float()
    u = ri(0, 16, (NG * 12, 64))
    I.gin = (u == 0).float() - (u == 1).float()            # density 1/8
    I.coef = torch.stack([torch.tensor([0.5, 1.0, 2.0])[ri(0, 3, (64,))], ri(-1, 2, (64,)).float(), ri(-2, 3, (64,)).float()])
    for k, v in list(vars(I).items()):
        setattr(I, k, v.to(DEV).contiguous())
    return I


@functools.lru_cache(maxsize=None)
def _gin_as(dtype, exp=None):
    """the gradient as the kernels read it: T, or the e5m2 bytes of value * 2^exp (the high byte of the float16 of a power of two)"""
    g = _inputs().gin
    if exp is None:
        return g.to(TORCH_T[dtype])
    half = (g * float(2 ** exp)).half()
    assert torch.equal(half.float(), g * float(2 ** exp))
    return ((half.view(torch.int16).int() >> 8) & 0xFF).to(torch.uint8)


# ---- the preconditions of "tolerance zero", asserted on the reference ------------------------------------------------------------
SEEN = {}


def _exact_values(tag, ref, dtype):
    """the values a kernel rounds to T are T numbers already"""
    assert torch.equal(ref, ref.to(TORCH_T[dtype]).double()), tag
    SEEN.setdefault(tag, {})["max |value|"] = float(ref.abs().max())


def _exact_stat(tag, name, terms, step=1.0):
    """a column sum of `terms` ([rows][columns]) is exact in float32 in any order and grouping: every term is an integer multiple of
    `step`, and even the column sums of |term| stay below 2^24 steps"""
    q = terms / step
    assert torch.equal(q, q.round()), (tag, name)
    top = float(q.abs().sum(0).max())
    assert top < 2 ** 24, (tag, name, top)
    SEEN.setdefault(tag, {})["sum |%s| / step" % name] = top


def _report(tag):
    print("\n[conv_exact] %s: %s (2^24 = 16777216)" % (tag, ", ".join("%s %g" % kv for kv in SEEN.get(tag, {}).items())))


# ---- the reference: float64, from the operation -----------------------------------------------------------------------------------
def _pad(t):
    """[N][12][C] -> [N][14][C]: a zero position on either side"""
    return torch.nn.functional.pad(t, (0, 0, 1, 1))


def _r1(lo, hi):
    """conv1 + ReLU of windows lo..hi-1: [n][12][64]"""
    I = _inputs()
    xp = torch.nn.functional.pad(I.x[lo:hi].double(), (1, 1))                       # [n][14]
    w = I.w1[:, 0, 1, :].double()                                                   # [64][3]
    y = I.b1.double() + sum(xp[:, t:t + 12, None] * w[None, None, :, t] for t in range(3))
    return torch.relu(y)


def _conv2(u1):
    """[N][12][64 in] -> [N][12][64 out]: 3-tap correlation over the zero-padded positions, plus the bias"""
    I = _inputs()
    w = I.w2[:, :, 1, :].double()                                                   # [o][c][tap]
    up = _pad(u1)
    return I.b2.double() + sum(up[:, t:t + 12, :] @ w[:, :, t].T for t in range(3))


def _conv2_dgrad(g):
    """the transposed correlation: g_v1[n][p][c] = sum_o sum_tap g[n][p - tap + 1][o] W2[o][c][tap]"""
    w = _inputs().w2[:, :, 1, :].double()
    gp = _pad(g)
    return sum(gp[:, 2 - t:14 - t, :] @ w[:, :, t] for t in range(3))


def _g(N):
    return _inputs().gin[:N * 12].double().view(N, 12, 64)


def _per_strip(rows, per):
    """[M][W] -> [strips][W]: the column sums of each group of `per` rows (the last one ragged)"""
    M, W = rows.shape
    n = -(-M // per)
    pad = torch.zeros(n * per, W, dtype=rows.dtype, device=rows.device)
    pad[:M] = rows
    return pad.view(n, per, W).sum(1)


def _dealt(per_strip, n):
    """what worker b of n holds when strip s goes to worker s % n: [n][...]"""
    m, rest = per_strip.shape[0], tuple(per_strip.shape[1:])
    k = -(-m // n)
    pad = torch.zeros((k * n,) + rest, dtype=per_strip.dtype, device=per_strip.device)
    pad[:m] = per_strip
    return pad.view((k, n) + rest).sum(0)


# ---- buffers and the launch -------------------------------------------------------------------------------------------------------
def _t_buffer(rows, dtype, fill=None):
    t = torch.empty(rows, 64, dtype=TORCH_T[dtype], device="cuda")
    if fill is not None:
        t.fill_(fill)
    elif dtype == BF16:
        t.view(torch.int16).fill_(SENT16)
    else:
        t.view(torch.int32).fill_(SENT32)
    return t


def _f_buffer(n):
    p = torch.empty(n, dtype=torch.float32, device="cuda")
    p.view(torch.int32).fill_(SENT32)
    return p


def _untouched(t):
    if t.dtype == torch.bfloat16:
        v = t.view(torch.int16)
        return torch.equal(v, torch.full_like(v, SENT16))
    v = t.view(torch.int32)
    return torch.equal(v, torch.full_like(v, SENT32))


def _launch(dtype, kind, N, gin=None, gin_exp=None, gcols=None, gcol_rows=0, out=None, partials=None, slabs=None, fold=None, dw=None, db=None):
    from contrastiveprosthetics_amd import _lib
    I = _inputs()
    d = _lib.cp_debug_conv_args()
    d.dtype, d.kind, d.n_windows = dtype, kind, N
    d.x, d.conv1_w, d.conv1_b, d.conv2_w, d.conv2_b = (t.data_ptr() for t in (I.x, I.w1, I.b1, I.w2, I.b2))
    d.stats1, d.coef = I.stats1.data_ptr(), I.coef.data_ptr()
    wc = torch.full((2 * SLAB,), NAN, dtype=TORCH_T[dtype], device="cuda")
    d.wc = wc.data_ptr()
    for name, t in (("gin", gin), ("gin_exp", gin_exp), ("gcols", gcols), ("out", out), ("partials", partials), ("slabs", slabs),
                    ("fold", fold), ("dw", dw), ("db", db)):
        setattr(d, name, t.data_ptr() if t is not None else None)
    d.gcol_rows = gcol_rows
    rows, grows = ctypes.c_int32(-1), ctypes.c_int32(-1)
    d.rows_out, d.gcol_rows_out = ctypes.pointer(rows), ctypes.pointer(grows)
    _lib.check(_lib.load().cp_debug_conv(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "cp_debug_conv")
    torch.cuda.synchronize()
    return rows.value, grows.value


def _where(got, ref, per):
    """which rows differ, in which strips (`per` rows each) and columns"""
    bad = got != ref
    rows = bad.any(-1).nonzero().flatten()
    cols = bad.any(0).nonzero().flatten()
    return "%d elements differ; rows %s .. %s (%d rows), strips %s, first columns %s" % (
        int(bad.sum()), rows[:8].tolist(), rows[-3:].tolist(), rows.numel(), torch.unique(rows // per)[:12].tolist(), cols[:8].tolist())


def _check_rows(tag, P, n, width, ref_rows):
    """the n partial rows of `width` floats at the head of P against ref_rows [n][width]; everything behind is untouched"""
    assert _untouched(P[n * width:]), (tag, "floats behind the last partial row were written")
    got = P[:n * width].view(n, width).double()
    assert torch.equal(got, ref_rows), (tag, "partial rows", _where(got, ref_rows, 1))


# ---- kind 0: conv1's statistics -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _conv1_chunk_sums(N, rpp):
    """[chunks][128]: sum and sum of squares of r1 over each `rpp` windows, and the precondition figures (values, |sum|, |sum of squares|)"""
    parts, top, a1, a2 = [], 0.0, 0, 0
    block = rpp * 256
    for lo in range(0, N, block):
        r = _r1(lo, min(lo + block, N)).reshape(-1, 64)
        assert torch.equal(r, r.round())
        top = max(top, float(r.max()))
        a1, a2 = a1 + r.sum(0), a2 + (r * r).sum(0)
        parts.append(torch.cat([_per_strip(r, rpp * 12), _per_strip(r * r, rpp * 12)], 1))
    return torch.cat(parts), top, float(a1.max()), float(a2.max())


@pytest.mark.parametrize("dtype,N", _cases(CONV1_N))
def test_conv1_statistics_are_exact(dtype, N):
    tag = "kind 0 %s N=%d" % (NAME_T[dtype], N)
    plan = host_plan(dtype, N)
    chunks, top, a1, a2 = _conv1_chunk_sums(N, plan["conv1_rpp"])
    assert top <= 4 and a2 < 2 ** 24, (tag, top, a2)                   # r1 >= 0: the column sums are the sums of |term|
    SEEN[tag] = {"max |value|": top, "sum |r1| / step": a1, "sum |r1^2| / step": a2}
    P = _f_buffer(P_FLOATS)
    g, _ = _launch(dtype, 0, N, partials=P)
    assert g == plan["g"], (tag, g, plan["g"])
    ref = _dealt(chunks, g)
    _check_rows(tag, P, g, 128, ref)
    if N <= 4096:
        whole = _r1(0, N).reshape(-1, 64)
        assert torch.equal(ref.sum(0), torch.cat([whole.sum(0), (whole * whole).sum(0)])), tag
    _report(tag)


# ---- kinds 1, 2 and 4: the strip kernels ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _strip_reference(N):
    I = _inputs()
    r1 = _r1(0, N)
    u1 = I.stats1[2].double() * r1 + I.stats1[3].double()
    fwd = torch.relu(_conv2(u1)).reshape(N * 12, 64)
    gv1 = _conv2_dgrad(_g(N))
    ca, cb, cz = (I.coef[i].double() for i in range(3))
    gy = torch.where(r1 > 0, ca * gv1 + cb * r1 + cz, torch.zeros_like(r1))
    xp = torch.nn.functional.pad(I.x[:N].double(), (1, 1))
    taps = [gy * xp[:, t:t + 12, None] for t in range(3)]                      # gy x[pos + tap - 1]
    return dict(r1=r1.reshape(N * 12, 64), u1=u1.reshape(N * 12, 64), fwd=fwd, gv1=gv1.reshape(N * 12, 64), gy=gy.reshape(N * 12, 64),
                taps=[t.reshape(N * 12, 64) for t in taps])


def _strip_case(tag, dtype, N, kind, ref, stats, steps, gin=None):
    """kinds 1 and 2: out and the partial rows, with the out buffer pre-filled with the NaN sentinel and with 1.0"""
    plan = host_plan(dtype, N)
    _exact_values(tag, ref, dtype)
    for (name, terms), step in zip(stats, steps):
        _exact_stat(tag, name, terms, step)
    ref_rows = _dealt(torch.cat([_per_strip(terms, 192) for _, terms in stats], 1), plan["grid"])
    for fill in (None, 1.0):
        out, P = _t_buffer(N * 12 + GUARD_ROWS, dtype, fill), _f_buffer(P_FLOATS)
        grid, _ = _launch(dtype, kind, N, gin=gin, out=out, partials=P)
        what = (tag, "out pre-filled with %s" % ("NaN" if fill is None else fill))
        assert grid == plan["grid"], (what, grid, plan["grid"])
        guard = out[N * 12:]
        assert _untouched(guard) if fill is None else bool((guard == fill).all()), (what, "rows behind N * 12 were written")
        got = out[:N * 12].double()
        assert torch.equal(got, ref), (what, _where(got, ref, 192))
        _check_rows(what, P, grid, 128, ref_rows)
        assert torch.equal(ref_rows.sum(0), torch.cat([terms.sum(0) for _, terms in stats])), what
    _report(tag)


@pytest.mark.parametrize("dtype,N", _cases(STRIP_N))
def test_conv2_forward_is_exact(dtype, N):
    tag = "kind 1 %s N=%d" % (NAME_T[dtype], N)
    R = _strip_reference(N)
    _exact_values(tag + " u1", R["u1"], dtype)
    assert float(R["r1"].max()) <= 4 and -1 <= float(R["u1"].min()) and float(R["u1"].max()) <= 9 and float(R["fwd"].max()) <= W2_NNZ * 9 + 3
    _strip_case(tag, dtype, N, 1, R["fwd"], [("v", R["fwd"]), ("v^2", R["fwd"] * R["fwd"])], [1.0, 1.0])


@pytest.mark.parametrize("dtype,N", _cases(STRIP_N))
def test_conv2_data_gradient_is_exact(dtype, N):
    tag = "kind 2 %s N=%d" % (NAME_T[dtype], N)
    R = _strip_reference(N)
    assert float(R["gv1"].abs().max()) <= 192
    _strip_case(tag, dtype, N, 2, R["gv1"], [("g", R["gv1"]), ("g r1", R["gv1"] * R["r1"])], [1.0, 1.0], gin=_gin_as(dtype))


def _fused_case(tag, dtype, N, gin, gin_exp=None):
    plan = host_plan(dtype, N)
    R = _strip_reference(N)
    _exact_values(tag + " r1", R["r1"], dtype)
    assert float(R["gy"].abs().max()) < 2 ** 10
    stats = [("gy x[tap %d]" % t, R["taps"][t]) for t in range(3)] + [("gy", R["gy"])]
    for name, terms in stats:
        _exact_stat(tag, name, terms, 0.5)
    ref_rows = _dealt(torch.cat([_per_strip(terms, 192) for _, terms in stats], 1), plan["grid"])
    P, fold, dw, db = _f_buffer(P_FLOATS), _f_buffer(32 * 256 + 4096), _f_buffer(64 * 9 + 1024), _f_buffer(64 + 1024)
    grid, _ = _launch(dtype, 4, N, gin=gin, gin_exp=gin_exp, partials=P, fold=fold, dw=dw, db=db)
    assert grid == plan["grid"], (tag, grid, plan["grid"])
    _check_rows(tag, P, grid, 256, ref_rows)
    if grid > 64:                                                         # the pre-reduce: row r goes to slice r % 32
        _check_rows(tag + " folded rows", fold, 32, 256, _dealt(ref_rows, 32))
    else:
        assert _untouched(fold), (tag, "the pre-reduce ran below 65 rows")
    total = ref_rows.sum(0).view(4, 64)
    assert torch.equal(total, torch.stack([terms.sum(0) for _, terms in stats])), tag
    assert _untouched(dw[64 * 9:]) and _untouched(db[64:]), (tag, "floats behind dW1 / db1 were written")
    got = dw[:64 * 9].view(64, 1, 3, 3).double()
    assert bool((got[:, :, 0, :] == 0).all()) and bool((got[:, :, 2, :] == 0).all()), (tag, "dW1 kernel rows 0 and 2")
    assert torch.equal(got[:, 0, 1, :], total[:3].T), (tag, "dW1 kernel row 1")
    assert torch.equal(db[:64].double(), total[3]), (tag, "db1")
    _report(tag)


@pytest.mark.parametrize("dtype,N", _cases(STRIP_N))
def test_conv2_dgrad_conv1_backward_is_exact(dtype, N):
    _fused_case("kind 4 %s N=%d" % (NAME_T[dtype], N), dtype, N, _gin_as(dtype))


@pytest.mark.parametrize("exp", [0, 3])
@pytest.mark.parametrize("N", [1, 17, 8193])
def test_conv2_dgrad_conv1_backward_from_e5m2_is_exact(N, exp):
    e = torch.tensor([exp], dtype=torch.int32, device="cuda")
    _fused_case("kind 4 e5m2 2^%d N=%d" % (exp, N), BF16, N, _gin_as(BF16, exp), e)


# ---- kind 3: the weight gradient ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _wgrad_reference(N):
    I = _inputs()
    r1, g = _r1(0, N), _g(N)
    s, t = I.stats1[2].double(), I.stats1[3].double()
    w = I.w2[:, :, 1, :].double()                                                  # [o][c][tap]
    strips = -(-N // 8)
    zeros = lambda a: torch.cat([a, torch.zeros((strips * 8 - N,) + a.shape[1:], dtype=a.dtype, device=a.device)])
    rp, gz = _pad(zeros(r1)).view(strips, 8, 14, 64), zeros(g).view(strips, 8, 12, 64)
    # P[strip][o][tap][c] = sum over the strip's windows and positions q of g[n][q][o] r1[n][q + tap - 1][c]
    P = torch.stack([torch.einsum("snqo,snqc->soc", gz, rp[:, :, tap:tap + 12, :]) for tap in range(3)], 2)
    Pabs = torch.stack([torch.einsum("nqo,nqc->oc", g.abs(), _pad(r1)[:, tap:tap + 12, :]) for tap in range(3)], 1)
    # dW2 from the operation: the correlation of g with u1 = s r1 + t, zero-padded AFTER the affine map
    up = _pad(s * r1 + t)
    dW2 = torch.stack([torch.einsum("nqo,nqc->oc", g, up[:, tap:tap + 12, :]) for tap in range(3)], 2)     # [o][c][tap]
    cols = g.sum(0)                                                                # [q][o]
    G = torch.stack([cols[1:].sum(0), cols.sum(0), cols[:11].sum(0)], 1)           # [o][tap]: the positions whose tap lands inside
    Pt = P.sum(0)                                                                  # [o][tap][c]
    rows2 = torch.stack([(w * G[:, None, :]).sum(2), (w * Pt.permute(0, 2, 1)).sum(2)], 1)      # [o][2][c]
    gv1 = _conv2_dgrad(g)
    return dict(P=P, Pabs=Pabs, dW2=dW2, G=G, rows2=rows2, g=g, S1=gv1.sum((0, 1)), S2=(gv1 * r1).sum((0, 1)), s=s, t=t)


def _gcols(N, nr):
    """caller rows [nr][768] of the gradient's column sums: row i holds the windows i, i + nr, ..; NaN behind"""
    g = _g(N).reshape(N, 768)
    room = torch.full((nr + 4, 768), NAN, device="cuda")
    room[:nr] = _dealt(g, nr).float()
    return room


def _wgrad_case(tag, dtype, N, gin, gin_exp=None, nrs=(None,) + tuple(GCOL_NR)):
    plan = host_plan(dtype, N)
    R = _wgrad_reference(N)
    S = plan["S"]
    _exact_stat(tag, "g r1", R["Pabs"].reshape(1, -1))                           # per entry of the product: the sum of |g r1|
    _exact_stat(tag, "g", R["g"].reshape(N, 768))
    assert torch.equal(R["dW2"], R["s"][None, :, None] * R["P"].sum(0).permute(0, 2, 1) + R["t"][None, :, None] * R["G"][:, None, :]), tag
    assert torch.equal(R["rows2"][:, 0].sum(0), R["S1"]) and torch.equal(R["rows2"][:, 1].sum(0), R["S2"]), tag
    assert float(R["dW2"].abs().max()) < 2 ** 24 and float(R["rows2"].abs().max()) < 2 ** 24
    ref_slabs = _dealt(R["P"].reshape(-1, SLAB), S)
    for nr in nrs:
        what = (tag, "colsum_kernel" if nr is None else "caller gcols, nr = %d" % nr)
        P, slabs, fold, dw = _f_buffer(P_FLOATS), _f_buffer((S + 32 + 2) * SLAB), _f_buffer(64 * 128 + 4096), _f_buffer(64 * 64 * 9 + 1024)
        gcols = None if nr is None else _gcols(N, nr)
        got_S, got_nr = _launch(dtype, 3, N, gin=gin, gin_exp=gin_exp, gcols=gcols, gcol_rows=nr or 0, partials=P, slabs=slabs, fold=fold, dw=dw)
        assert got_S == S, (what, got_S, S)
        if nr is None:
            assert got_nr == plan["gcol_rows"], (what, got_nr, plan["gcol_rows"])
            rpp = 2 if dtype == BF16 else 1                                         # colsum_kernel: rpp windows per block and pass
            _check_rows(what, P, got_nr, 768, _dealt(_per_strip(R["g"].reshape(N, 768), rpp), got_nr))
        else:
            assert got_nr == nr and _untouched(P), (what, got_nr)
        n_slabs = S + 32 if S > 64 else S
        assert _untouched(slabs[n_slabs * SLAB:]), (what, "floats behind the last slab were written")
        got = slabs[:S * SLAB].view(S, SLAB).double()
        assert torch.equal(got, ref_slabs), (what, "slabs", _where(got, ref_slabs, 1))
        if S > 64:
            got = slabs[S * SLAB:n_slabs * SLAB].view(32, SLAB).double()
            ref = _dealt(ref_slabs, 32)
            assert torch.equal(got, ref), (what, "folded slabs", _where(got, ref, 1))
        assert torch.equal(ref_slabs.sum(0), R["P"].sum(0).reshape(-1)), what
        assert _untouched(dw[64 * 64 * 9:]) and _untouched(fold[64 * 128:]), (what, "floats behind dW2 / rows2 were written")
        got = dw[:64 * 64 * 9].view(64, 64, 3, 3).double()
        assert bool((got[:, :, 0, :] == 0).all()) and bool((got[:, :, 2, :] == 0).all()), (what, "dW2 kernel rows 0 and 2")
        assert torch.equal(got[:, :, 1, :], R["dW2"]), (what, "dW2 kernel row 1", int((got[:, :, 1, :] != R["dW2"]).sum()))
        got = fold[:64 * 128].view(64, 2, 64).double()
        assert torch.equal(got, R["rows2"]), (what, "rows2", int((got != R["rows2"]).sum()))
    _report(tag)


@pytest.mark.parametrize("dtype,N", _cases(WGRAD_N))
def test_conv2_weight_gradient_is_exact(dtype, N):
    _wgrad_case("kind 3 %s N=%d" % (NAME_T[dtype], N), dtype, N, _gin_as(dtype))


@pytest.mark.parametrize("exp", [0, 3])
@pytest.mark.parametrize("N", [1, 17, 4097])
def test_conv2_weight_gradient_from_e5m2_is_exact(N, exp):
    e = torch.tensor([exp], dtype=torch.int32, device="cuda")
    _wgrad_case("kind 3 e5m2 2^%d N=%d" % (exp, N), BF16, N, _gin_as(BF16, exp), e, nrs=tuple(GCOL_NR))
