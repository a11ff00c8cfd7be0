"""The L2 + Adam kernels (csrc/optim.cuh: l2_sumsq_kernel, l2_finalize_kernel, adam_kernel<true>, and the host code under
"optimiser" in csrc/api.hip) called on their own -- cp_l2_adam_step, cp_l2_adam_step_graph and cp_l2_norms through _lib.load()
with this module's own tensor tables, no Engine, no encoder -- against the float64 reference of oracle/optim_cpu.py (itself pinned
against torch.optim.Adam by tests/test_oracle_optim.py).

Inputs (seeded, float32, handed to the reference widened; "unit-normal" with magnitudes under 1e-3 raised to 1e-3, so that the
smallest intermediate, the second moment of an element whose only gradient is the regulariser's, stays above 1e-30).  p is
unit-normal times 10^u, u uniform in [-3, 1]; g unit-normal times
10^[-4, 0] with element 3 of every 7 of a tensor exactly 0; m is 1e-2 times unit-normal and v its square, both exactly 0 at element
3 of every 21 (so a tensor outside the regulariser has elements with zero g, m and v: they must not move).  Every case asserts on
the float64 side that no non-zero intermediate leaves [1e-30, 1e30].  lr = (1e-3, 3e-2), reg = (1e-3, 2e-2), beta = 0.9 / 0.999,
eps = 1e-8.  In this module's own tables neighbouring tensors differ in group, every second pair also in regulariser membership
(the pattern (0, member), (1, no), (0, no), (1, member)), and in every table neighbouring norms differ by at least a factor of 2
(a tensor is scaled by 1/4 where chance put it closer): a chunk handed its neighbour's tensor fails.  A member with several chunks
and a ragged last one has its final element set so that the last chunk carries at least 1e-3 of the squared norm: a skipped tail
shows in the regulariser value.  The four flat buffers, the scratch and the l2_out scalar have a margin in front, behind and
between tensors; every float outside the table holds the NaN pattern 0x7FC0BEEF and is compared bit for bit afterwards.

Tables (all of this module's own together hold under 0.6 M floats, the two model tables 2.0 M each):
    model-stock, model-adabn     Engine's parameter specs (one-hot / glove class encoder), 256-byte aligned: the path the step runs
    packed, packed-rot           no alignment, numel 1, 2, 3, 4, 5, 7, 2047, 2048, 2049, 4096, 4097, 2048*17+1: the scalar branch
                                 of both kernels, tails of 1, 18 chunks over 16 fold lanes (-rot: the membership pattern moved on by
                                 two, so that every size is a member once)
    mixed                        offsets a multiple of 4 with numel 4, 8, 2044, 2052, 393,220 (192 chunks + one float4) between
                                 odd-sized tensors: both branches in one launch
    t64, n1                      64 tensors (CP_MAX_TENSORS) with a zero-length tensor in the middle and one as the last entry; one
                                 tensor: the binary search's ends, block 0's four passes over the norm table, all 1024 threads of
                                 l2_finalize_kernel
    mixed-shift-all / -g / -p    base pointers one float off: the pointer half of the path choice.  With g alone shifted adam_kernel
                                 takes its scalar branch on the numbers the vector branch saw: p, m, v bit-identical to `mixed`
    zero, zero-reg0              all-zero members of 2048 (vector branch) and 5 (scalar) elements; -reg0: reg_emg = 0 (0 / 0)
    packed-gs8                   grad_scale = 1/8
    steps                        `packed`, steps 1, 2, 3 with the state carried on the device, then step 1000
    graph                        cp_l2_adam_step_graph on `mixed`, captured once, replayed for steps 1..3 with the device
                                 cp_step_state rewritten in between: bit-identical to cp_l2_adam_step
Every single-step case also runs cp_l2_norms first: it leaves p alone and its l2_out is bit-identical to the step's.

Metrics, every element of every tensor.
    m (exp_avg)       |m - ref| over m_scale = beta1 |m_old| + (1 - beta1) (|grad_scale g| + |reg p / |p||)     (m can cancel)
    v (exp_avg_sq)    |v - ref| over ref                                                          (all terms non-negative)
    p                 (|p - ref| - 2^-24 |ref|) over p_scale = (lr / bc1) m_scale / (sqrt(v_ref) / sqrt(bc2) + eps); the second
                      term is the one rounding of the stored result
    where m_scale = 0 p is bit-identical and m is exactly 0; where v_ref = 0, v is exactly 0
    regulariser       2e-6 relative (the bar of tests/test_gpu_parity.py::test_l2_adam_kernel_matches_torch)
    outside           bit-identical

Bars.  Each of the three is 4 x the worst value that the reference's float32 mode (plain torch float32, same formulas) shows
against its float64 mode on this module's inputs over all its cases, measured on the CPU (`python -m tests.test_gpu_optim`
from the repository root prints them; the steps case carries the float32 mode's state there):
    M_BASELINE 1.75e-7 (model-adabn)   V_BASELINE 3.69e-7 (model-stock)   U_BASELINE 3.20e-7 (mixed, step 2)
    M_BAR      7.0e-7                  V_BAR      1.48e-6                 U_BAR      1.28e-6
(the smallest case, n1, shows 1.3e-7 / 1.9e-7 / 2.0e-7: the figures are roundings per element, not sums, and barely grow with size)
The factor 4 is for the roundings a kernel may order differently: fmaf, 1 / sqrtf(bc2) formed once, chunked sums.

Sensitivity, asserted in every case on the reference alone (float32 mode against float64 mode): the float32 mode passes; with the
last element of a ragged tensor left un-updated it fails the parameter check; with the first chunk of one tensor computed from its
neighbour's lr, reg and norm it fails the parameter check (not in n1: no neighbour); a regulariser value summed without one
member's last chunk misses the 2e-6 bar.

Measured on the device (MI355X): worst element of a case (every case prints its own line)

    case                                   m         v         U         regulariser rel
    model-stock / model-adabn              1.64e-07  3.20e-07  2.20e-07  3.6e-08
    packed / packed-rot / packed-gs8       1.39e-07  2.58e-07  1.91e-07  2.8e-08
    mixed (= mixed-shift-g, bit for bit)   1.75e-07  3.72e-07  2.15e-07  3.4e-08
    mixed-shift-all / mixed-shift-p        1.54e-07  2.49e-07  1.93e-07  3.4e-08
    t64 / n1                               1.74e-07  3.60e-07  2.01e-07  7.8e-08
    zero / zero-reg0                       1.30e-07  2.05e-07  1.54e-07  3.2e-08
    steps 1, 2, 3, 1000                    2.01e-07  2.93e-07  2.20e-07  3.5e-08
                       bar                 7.0e-07   1.48e-06  1.28e-06  2e-6
                       float32 torch       1.75e-07  3.69e-07  3.20e-07

The kernels sit at the float32 torch baseline (m 1.15 x, v 1.01 x, U 0.69 x of it).  In every case the elements that must not
move did not, nothing outside the tables was written, cp_l2_norms' value equalled the step's bit for bit, and the graph form
replayed bit-identical to the plain step at steps 1, 2, 3; the whole module takes 3.3 s.

What the module found.  (1) A member of the regulariser whose norm is 0: adam_kernel formed reg / 0 * 0 = NaN, and the parameter
and both moments of the whole tensor were NaN from then on (`zero`, `zero-reg0`: 297 non-finite floats before the change); such a
member now takes no regulariser gradient, as torch.norm's gradient at the zero tensor is 0.  (2) adam_kernel's two branches were
NOT the same numbers: the compiler had contracted `beta * m + (1 - beta) * g` differently in each (the vector branch
fmaf(beta, m, (1 - beta) g) for both moments; the scalar branch fmaf(1 - beta1, g, beta1 m) and an unfused second moment), so
`mixed-shift-g` differed from `mixed` in p, m and v.  The update is now written with explicit fmaf in the vector branch's form --
the one every tensor of the model takes, whose instructions did not change.  (3) build_opt took any table: a negative numel or
offset is refused now, as is a table without an element (tests/test_cabi_and_host.py).
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import optim_cpu as oc

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC0BEEF
CHUNK, LANES, MAX_TENSORS = 2048, 16, 64
HYPER = dict(lr_emg=1e-3, lr_glove=3e-2, reg_emg=1e-3, reg_glove=2e-2, beta1=0.9, beta2=0.999, eps=1e-8)
L2_BAR = 2e-6
M_BASELINE, V_BASELINE, U_BASELINE = 1.75e-7, 3.69e-7, 3.20e-7
M_BAR, V_BAR, U_BAR = 4 * M_BASELINE, 4 * V_BASELINE, 4 * U_BASELINE
ROUND = 2.0 ** -24
PATTERN4 = ((0, 1), (1, 0), (0, 0), (1, 1))                       # (group, member) of tensor i % 4


# ------------------------------------------------------------------------------------------------ tables
class Table:
    def __init__(self, rows, zero_rows=()):
        self.rows = [tuple(int(x) for x in r) for r in rows]      # (offset, numel, group, l2)
        self.zero_rows = tuple(zero_rows)
        end = 0
        for off, n, _, _ in self.rows:
            assert off >= end, "tables of this module do not overlap"
            end = off + n
        self.length = end + 37                                    # margin behind
        self.mask = torch.zeros(self.length, dtype=torch.bool)
        self.eidx = torch.full((self.length,), -1, dtype=torch.int64)
        for off, n, _, _ in self.rows:
            self.mask[off:off + n] = True
            self.eidx[off:off + n] = torch.arange(n)

    def vector(self, i, shifted=False):
        """the tensor's half of the kernels' path choice"""
        off, n = self.rows[i][:2]
        return ((off | n) & 3) == 0 and not shifted

    def chunks(self, i):
        return (self.rows[i][1] + CHUNK - 1) // CHUNK

    def ctypes(self):
        n = len(self.rows)
        col = lambda k, t: (t * n)(*[r[k] for r in self.rows])
        return col(0, C.c_int64), col(1, C.c_int64), col(2, C.c_int32), col(3, C.c_int32), n


def place(sizes, front, gap, align=lambda i: 1, pattern=0, kinds=None):
    rows, end = [], front
    for i, n in enumerate(sizes):
        a = align(i)
        off = (end + (gap(i) if i else 0) + a - 1) // a * a
        grp, l2 = kinds[i] if kinds else PATTERN4[(i + pattern) % 4]
        rows.append((off, n, grp, l2))
        end = off + n
    return rows


PACKED = (1, 2, 3, 4, 5, 7, 2047, 2048, 2049, 4096, 4097, 2048 * 17 + 1)
MIXED = (4, 3, 8, 5, 2044, 2047, 2052, 2049, 393220, 4097)
T64 = tuple([1, 6, 64, 300, 2048, 2050, 4100, 777, 12, 5000, 3, 2047, 128, 4096, 33, 2049][i % 16] + (i // 16) for i in range(64))


@functools.lru_cache(maxsize=None)
def table(name):
    if name.startswith("model"):
        from contrastiveprosthetics_amd.engine import l2_member, param_specs
        specs = param_specs(name == "model-adabn", class_encoder="glove" if name == "model-adabn" else "onehot")
        sizes = [int(torch.Size(s).numel()) for s in specs.values()]
        kinds = [(1 if k.startswith("glove_net.") else 0, 1 if l2_member(k) else 0) for k in specs]
        t = Table(place(sizes, 64, lambda i: 64, lambda i: 64, kinds=kinds))
        assert all(t.vector(i) for i in range(len(sizes))) and len(sizes) <= MAX_TENSORS
        return t
    if name in ("packed", "packed-rot"):
        t = Table(place(PACKED, 5, lambda i: 0 if i % 2 else 3, pattern=2 if name == "packed-rot" else 0))
        assert not any(t.vector(i) for i in range(len(PACKED)))                              # the scalar branch throughout
        assert t.chunks(len(PACKED) - 1) == 18 > LANES
        return t
    if name == "mixed":
        t = Table(place(MIXED, 8, lambda i: 1 if MIXED[i] % 4 else 4, lambda i: 1 if MIXED[i] % 4 else 4))
        assert [t.vector(i) for i in range(len(MIXED))] == [n % 4 == 0 for n in MIXED]
        assert MIXED[8] == 192 * CHUNK + 4
        return t
    if name == "t64":
        sizes = list(T64)
        sizes[31] = sizes[63] = 0
        t = Table(place(sizes, 3, lambda i: (0, 1, 4, 2)[i % 4], lambda i: 4 if i % 3 == 0 else 1))
        assert len(t.rows) == MAX_TENSORS and any(t.vector(i) for i in range(64)) and not all(t.vector(i) for i in range(64))
        return t
    if name == "n1":
        return Table([(6, 4099, 1, 1)])
    if name == "zero":
        #           offset, numel, group, l2
        return Table([(4, 300, 0, 1), (320, 2048, 1, 1), (2371, 777, 0, 0), (3150, 5, 0, 1), (3157, 12, 1, 0), (3172, 2050, 1, 1)],
                     zero_rows=(1, 3))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(name, seed=0):
    """p, g, m, v: float32 CPU buffers of the table's length, the NaN pattern outside the table.  Never modified."""
    t = table(name)
    gen = torch.Generator().manual_seed(4000 + seed + sum(ord(c) for c in name))
    L = t.length
    def normal():                                                 # unit-normal, no magnitude under 1e-3 (nothing is left to chance)
        x = torch.randn(L, generator=gen)
        return torch.where(x.abs() < 1e-3, torch.copysign(torch.full_like(x, 1e-3), x), x)

    scaled = lambda lo, hi: normal() * 10.0 ** ((hi - lo) * torch.rand(L, generator=gen) + lo)
    p, g, m = scaled(-3, 1), scaled(-4, 0), 1e-2 * normal()
    g[t.eidx % 7 == 3] = 0
    m[t.eidx % 21 == 3] = 0
    prev = None
    for i, (off, n, grp, l2) in enumerate(t.rows):
        x = p[off:off + n]
        if i in t.zero_rows:
            x.zero_()
            continue
        if n == 0:
            continue
        tail = n % CHUNK
        if l2 and n > CHUNK and tail:
            total = float(x.double().pow(2).sum())
            if float(x[n - tail:].double().pow(2).sum()) < 2e-3 * total:
                x[n - 1] = (2e-3 * total) ** 0.5
            total = float(x.double().pow(2).sum())
            assert float(x[n - tail:].double().pow(2).sum()) >= 1e-3 * total
        norm = float(x.double().norm())
        if prev is not None and 0.5 < norm / prev < 2.0:
            x *= 0.25
            norm = float(x.double().norm())
        assert prev is None or not 0.5 <= norm / prev <= 2.0
        prev = norm
    v = m * m
    for x in (p, g, m, v):
        x.view(torch.int32)[~t.mask] = PATTERN
    return dict(p=p, g=g, m=m, v=v)


def gradient(name, step):
    """the gradient of a later step: as inputs()'s g, another seed"""
    return inputs(name, seed=100 * step)["g"]


def reference(name, inp, hyper, grad_scale, step, dtype=torch.float64, **kw):
    t = table(name)
    return oc.l2_adam_reference(inp["p"].double(), inp["g"].double(), inp["m"].double(), inp["v"].double(), t.rows, hyper,
                                grad_scale=grad_scale, step=step, dtype=dtype, **kw)


# ------------------------------------------------------------------------------------------------ the comparison
def errors(t, got, ref, before):
    """worst m, v and U figure over every element of the table, and the number of elements that had to be exact and are not.
    got: p, m, v (flat, any float dtype); ref: the float64 reference's result; before: the inputs of the step."""
    ms, ps, rv = ref["m_scale"], ref["p_scale"], ref["v"]
    live, still = t.mask & (ms > 0), t.mask & (ms == 0)
    worst = lambda x: float(x.max()) if x.numel() else 0.0                       # (NaN propagates)
    gp, gm, gv = got["p"].double(), got["m"].double(), got["v"].double()
    fig = dict(m=worst((gm - ref["m"]).abs()[live] / ms[live]))
    pos = t.mask & (rv > 0)
    fig["v"] = worst((gv - rv).abs()[pos] / rv[pos])
    excess = ((gp - ref["p"]).abs() - ROUND * ref["p"].abs()).clamp(min=0)
    fig["U"] = worst(excess[live] / ps[live])
    moved = got["p"].float().view(torch.int32)[still] != before["p"].view(torch.int32)[still]
    fig["inexact"] = int(moved.sum()) + int((gm[still] != 0).sum()) + int((gv[t.mask & (rv == 0)] != 0).sum())
    return fig


def within(fig):
    return fig["m"] <= M_BAR and fig["v"] <= V_BAR and fig["U"] <= U_BAR and fig["inexact"] == 0


def check_extent(ref):
    lo, hi = ref["extent"]
    assert 1e-30 <= lo and hi <= 1e30, (lo, hi)


def sensitivity(name, inp, hyper, grad_scale, step, ref):
    """on the reference alone: its float32 mode passes the bars, and three corruptions of it do not.  -> the float32 mode's figures"""
    t = table(name)
    f32 = reference(name, inp, hyper, grad_scale, step, dtype=torch.float32)
    base = errors(t, f32, ref, inp)
    assert within(base), ("the float32 reference misses the bars", base)
    live = [i for i, r in enumerate(t.rows) if r[1] > 0]
    # (a) the last element of a ragged tensor left as it was
    ragged = [i for i in live if t.rows[i][1] % CHUNK and float(ref["p_scale"][t.rows[i][0] + t.rows[i][1] - 1]) > 0]
    i = max(ragged, key=lambda i: (t.rows[i][3], t.rows[i][1]))                  # a member if there is one, the largest
    bad = dict(f32, p=f32["p"].clone())
    last = t.rows[i][0] + t.rows[i][1] - 1
    bad["p"][last] = inp["p"][last]
    assert errors(t, bad, ref, inp)["U"] > U_BAR, "an un-updated last element would pass"
    # (b) the first chunk of one tensor with its neighbour's lr, reg and norm
    if len(live) > 1:
        i = max(live, key=lambda i: t.rows[i][1])
        j = [k for k in live if k != i and float(f32["norms"][k]) > 0]
        j = min(j, key=lambda k: abs(k - i))
        off, n, _, l2 = t.rows[i]
        span = min(n, CHUNK)
        sub = oc.l2_adam_reference(inp["p"].double(), inp["g"].double(), inp["m"].double(), inp["v"].double(),
                                   [(off, span, t.rows[j][2], l2)], hyper, grad_scale=grad_scale, step=step,
                                   norms=[float(f32["norms"][j])], dtype=torch.float32)
        bad = {k: f32[k].clone() for k in ("p", "m", "v")}
        for k in bad:
            bad[k][off:off + span] = sub[k][off:off + span]
        assert errors(t, bad, ref, inp)["U"] > U_BAR, "a first chunk computed with the neighbour's parameters would pass"
    # (c) the regulariser value without one member's last chunk
    value, reg, dev = float(ref["l2"]), (oc.as_float32(hyper["reg_emg"]), oc.as_float32(hyper["reg_glove"])), 0.0
    for i in live:
        off, n, grp, l2 = t.rows[i]
        if l2 and n % CHUNK:
            x = inp["p"][off:off + n].double()
            short = float(x[:n - n % CHUNK].norm())
            dev = max(dev, reg[grp] * (float(x.norm()) - short) / value)
    assert dev > L2_BAR, "a skipped last chunk would pass the regulariser bar"
    return base


# ------------------------------------------------------------------------------------------------ the device side
class Device:
    """the four flat buffers, scratch and l2_out of one table on the GPU, every float outside the table the NaN pattern"""

    def __init__(self, name, shift=(), grad_scale=1.0, hyper=HYPER):
        from contrastiveprosthetics_amd import _lib
        self.lib, self._lib, self.t, self.shift = _lib.load(), _lib, table(name), tuple(shift)
        L = self.t.length
        self.raw = {k: torch.empty(L + 8, dtype=torch.float32, device="cuda") for k in "pgmv"}
        self.at = {k: (5 if k in self.shift else 4) for k in "pgmv"}             # where the table's float 0 lies in raw
        for k, r in self.raw.items():
            assert r.data_ptr() % 256 == 0
        self.view = {k: self.raw[k][self.at[k]:self.at[k] + L] for k in "pgmv"}
        self.tab = self.t.ctypes()
        self.n_scratch = int(self.lib.cp_optimizer_scratch_floats(self.tab[1], self.tab[4]))
        assert self.n_scratch >= sum(self.t.chunks(i) for i in range(len(self.t.rows))) + len(self.t.rows)
        self.scratch = torch.empty(self.n_scratch + 64, dtype=torch.float32, device="cuda")
        self.l2 = torch.empty(3, dtype=torch.float32, device="cuda")
        self.h = _lib.cp_adam_hyper(hyper["lr_emg"], hyper["lr_glove"], hyper["reg_emg"], hyper["reg_glove"], hyper["beta1"],
                                    hyper["beta2"], hyper["eps"], grad_scale)

    def load(self, inp, only=None):
        for k in only or "pgmv":
            self.raw[k].view(torch.int32).fill_(PATTERN)
            self.view[k].copy_(inp[k])
        if only is None:
            self.scratch.view(torch.int32).fill_(PATTERN)
            self.l2.view(torch.int32).fill_(PATTERN)

    def _ptr(self, k):
        return self.view[k].data_ptr()

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def norms(self):
        self._lib.check(self.lib.cp_l2_norms(self._ptr("p"), *self.tab, C.byref(self.h), self.scratch.data_ptr(),
                                             self.l2.data_ptr() + 4, self._stream()), "cp_l2_norms")

    def step(self, step):
        self._lib.check(self.lib.cp_l2_adam_step(self._ptr("p"), self._ptr("g"), self._ptr("m"), self._ptr("v"), *self.tab,
                                                 C.byref(self.h), step, self.scratch.data_ptr(), self.l2.data_ptr() + 4,
                                                 self._stream()), "cp_l2_adam_step")

    def step_graph(self, state):
        self._lib.check(self.lib.cp_l2_adam_step_graph(self._ptr("p"), self._ptr("g"), self._ptr("m"), self._ptr("v"), *self.tab,
                                                       C.byref(self.h), state.data_ptr(), self.scratch.data_ptr(),
                                                       self.l2.data_ptr() + 4, self._stream()), "cp_l2_adam_step_graph")

    def read(self):
        """-> p, g, m, v as CPU buffers of the table's length, the regulariser value, and the number of floats outside the table
        (margins of the six buffers included) that no longer hold the pattern"""
        torch.cuda.synchronize()
        out, touched = {}, 0
        L = self.t.length
        for k in "pgmv":
            raw = self.raw[k].cpu()
            out[k] = raw[self.at[k]:self.at[k] + L].clone()
            bits = raw.view(torch.int32).clone()
            bits[self.at[k]:self.at[k] + L][self.t.mask] = PATTERN
            touched += int((bits != PATTERN).sum())
        touched += int((self.scratch[self.n_scratch:].cpu().view(torch.int32) != PATTERN).sum())
        l2 = self.l2.cpu()
        touched += int((l2.view(torch.int32)[[0, 2]] != PATTERN).sum())
        out["l2"] = l2[1].clone()
        return out, touched


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def judge(label, t, got, touched, ref, before, extra=()):
    """prints the case's figures, then asserts them"""
    fig = errors(t, got, ref, before)
    fig["l2 rel"] = abs(float(got["l2"]) - float(ref["l2"])) / float(ref["l2"])
    fig["outside"] = touched + (0 if same_bits(got["g"], before["g"]) else 1)
    finite = all(bool(torch.isfinite(got[k][t.mask]).all()) for k in "pmv")
    print(f"\noptim {label:22s} tensors {len(t.rows):2d} floats {int(t.mask.sum()):8d} | m {fig['m']:.2e}  v {fig['v']:.2e}  "
          f"U {fig['U']:.2e}  l2 rel {fig['l2 rel']:.2e}  inexact {fig['inexact']}  outside {fig['outside']}"
          + "".join(f"  {k} {x}" for k, x in extra) + ("" if finite else "  NON-FINITE"))
    fails = [f"{k} {fig[k]:.3e} > {bar:.1e}" for k, bar in (("m", M_BAR), ("v", V_BAR), ("U", U_BAR), ("l2 rel", L2_BAR))
             if not fig[k] <= bar]
    fails += [f"{k}: {fig[k]} floats" for k in ("inexact", "outside") if fig[k]]
    fails += [f"{k}: {x}" for k, x in extra if x]
    assert finite, "non-finite parameters or moments: " + "; ".join(fails)
    assert not fails, "; ".join(fails)
    return fig


#        id, table, shifted buffers, grad_scale, hyper
CASES = [(n, n, (), 1.0, HYPER) for n in ("model-stock", "model-adabn", "packed", "packed-rot", "mixed", "t64", "n1")] + \
        [("mixed-shift-all", "mixed", "pgmv", 1.0, HYPER), ("mixed-shift-g", "mixed", "g", 1.0, HYPER),
         ("mixed-shift-p", "mixed", "p", 1.0, HYPER),
         ("zero", "zero", (), 1.0, HYPER), ("zero-reg0", "zero", (), 1.0, dict(HYPER, reg_emg=0.0)),
         ("packed-gs8", "packed", (), 0.125, HYPER)]
STEPS = (1, 2, 3, 1000)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_step_against_float64(case):
    label, name, shift, grad_scale, hyper = case
    t, inp = table(name), inputs(name)
    ref = reference(name, inp, hyper, grad_scale, 1)
    check_extent(ref)
    sensitivity(name, inp, hyper, grad_scale, 1, ref)
    if name == "zero":
        for i in t.zero_rows:
            off, n = t.rows[i][:2]
            assert float(ref["norms"][i]) == 0 and bool(torch.isfinite(ref["p"][off:off + n]).all())
    d = Device(name, shift, grad_scale, hyper)
    d.load(inp)
    d.norms()
    alone, touched = d.read()
    extra = [("cp_l2_norms wrote p", 0 if same_bits(alone["p"], inp["p"]) else 1), ("cp_l2_norms outside", touched)]
    d.step(1)
    got, touched = d.read()
    extra.append(("l2_out differs from cp_l2_norms", 0 if same_bits(got["l2"], alone["l2"]) else 1))
    if label == "mixed-shift-g":
        # adam_kernel's two branches are the same arithmetic: with g alone off by a float, the scalar branch on the vector
        # branch's norms
        e = Device(name, (), grad_scale, hyper)
        e.load(inp)
        e.step(1)
        straight, _ = e.read()
        extra.append(("bits differ from the unshifted run", sum(0 if same_bits(got[k], straight[k]) else 1 for k in ("p", "m", "v", "l2"))))
    judge(label, t, got, touched, ref, inp, extra)


def test_steps_carry_state_and_bias_corrections():
    """steps 1, 2, 3 with the moments and parameters left on the device, a new gradient each, then step 1000 on that state:
    every step against the reference applied to what the device held before it"""
    name = "packed"
    t, d = table(name), Device(name)
    d.load(inputs(name))
    for step in STEPS:
        before, _ = d.read()
        before["g"] = gradient(name, step)
        d.load(before, only="g")
        ref = reference(name, before, HYPER, 1.0, step)
        check_extent(ref)
        sensitivity(name, before, HYPER, 1.0, step, ref)
        d.step(step)
        got, touched = d.read()
        judge(f"steps: step {step}", t, got, touched, ref, before)


def test_graph_form_replays_bit_identical_to_the_plain_step():
    """cp_l2_adam_step_graph reads bc1, bc2 and the learning rates from a device cp_step_state: captured once (its two launches in
    a line), replayed for steps 1..3 with the state rewritten between replays, against cp_l2_adam_step on a second set of
    buffers"""
    name = "mixed"
    inp = inputs(name)
    plain, graphed = Device(name), Device(name)
    state = torch.zeros(8, dtype=torch.float32, device="cuda")            # cp_step_state: dp_salt, bc1, bc2, lr_emg, lr_glove, pad
    graphed.load(inp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                         # once outside the capture (module load)
        graphed.step_graph(state)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_graph(state)
    plain.load(inp)
    graphed.load(inp)
    differ = 0
    for step in (1, 2, 3):
        if step > 1:
            grad = dict(g=gradient(name, step))
            plain.load(grad, only="g")
            graphed.load(grad, only="g")
        bc1, bc2 = oc.bias_corrections(HYPER["beta1"], HYPER["beta2"], step)
        state.copy_(torch.tensor([0.0, bc1, bc2, HYPER["lr_emg"], HYPER["lr_glove"], 0.0, 0.0, 0.0], dtype=torch.float32))
        g.replay()
        plain.step(step)
        a, ta = plain.read()
        b, tb = graphed.read()
        bad = [k for k in ("p", "m", "v", "l2") if not same_bits(a[k], b[k])]
        print(f"\noptim graph: step {step}            differing buffers {bad or 'none'}  outside {ta + tb}")
        differ += len(bad) + ta + tb
        assert bool(torch.isfinite(b["p"][table(name).mask]).all())
    assert differ == 0


# ------------------------------------------------------------------------------------------------ the float32 baselines (CPU)
def measure_baselines():
    """the worst m, v and U figure of the reference's float32 mode against its float64 mode over this module's cases"""
    worst = dict(m=0.0, v=0.0, U=0.0)

    def one(label, name, inp, hyper, grad_scale, step):
        ref = reference(name, inp, hyper, grad_scale, step)
        f32 = reference(name, inp, hyper, grad_scale, step, dtype=torch.float32)
        fig = errors(table(name), f32, ref, inp)
        print(f"{label:22s} m {fig['m']:.3e}  v {fig['v']:.3e}  U {fig['U']:.3e}  inexact {fig['inexact']}  "
              f"l2 rel {abs(float(f32['l2']) - float(ref['l2'])) / float(ref['l2']):.2e}  extent {ref['extent'][0]:.1e} .. {ref['extent'][1]:.1e}")
        for k in worst:
            worst[k] = max(worst[k], fig[k])
        return f32

    for label, name, shift, grad_scale, hyper in CASES:
        if not shift:
            one(label, name, inputs(name), hyper, grad_scale, 1)
    for name, steps in (("packed", STEPS), ("mixed", (1, 2, 3))):
        cur = dict(inputs(name))
        for step in steps:
            if step > 1:
                cur["g"] = gradient(name, step)
            f32 = one(f"{name}: step {step}", name, cur, HYPER, 1.0, step)
            cur = dict(cur, **{k: f32[k] for k in ("p", "m", "v")})
    print("baselines: " + "  ".join(f"{k} {x:.3e} (x 4 = {4 * x:.3e})" for k, x in worst.items()))


if __name__ == "__main__":
    measure_baselines()
