"""The contrastive head kernel (csrc/head.cuh: head_kernel in its f32 / bf16, one-hot / glove / global-negatives / 8-bit-logits
instantiations, head_finalize_kernel, and reduce_rows_kernel in front of it) called on its own -- z, a class table and labels, no
encoder -- against the float64 reference of oracle/head_cpu.py (itself pinned by tests/test_oracle_head.py).

What each case reads: the logits, the loss, the correct count, every prediction, dL/dz row by row through cp_debug_head_grad (all
64 columns of every row), dL/dzg through cp_debug_glove_head_grad, and the class-table gradients.

Inputs.  z rows are unit-normal times 10^u, u uniform in [-3, 3]: the logits do not see |z|, dL/dz scales as 1/|z|, so the kernel's
1/|z| factor shows row by row.  The class columns easy_w[:, c] have lengths spread over [0.5, 2], easy_b is non-zero; glove rows zg
carry their own scales 10^[-2, 2].  The workspace (and the glove workspace) is filled with 0xFF bytes before every call and the
gradient store with NaN: head_kernel and head_finalize_kernel read back from the workspace only the partial rows they wrote
(reduce_rows_kernel also folds the 46 padding columns of each 704-wide partial row, which nothing reads afterwards), so an element
the kernels fail to write comes back NaN and fails its comparison.  (CP_FP8 workspaces keep their scale table, the first KiB.)

Group counts (V = 1 unless said): where the launch changes shape --
    1, 5            one block, idle waves
    256 | 257       64 | 65 blocks: head_finalize_kernel reads the partial rows itself | reduce_rows_kernel's pre-reduction
    2047 | 2048     one | two groups per wave (LDS tiles and the per-wave dE accumulator reused behind wave barriers)
    2049            two per wave with a ragged tail
    8193            the grid capped at 1024 blocks: one wave takes a third group (bf16; a 4 GB workspace)
    B = 2, V = 3    gradients at V > 1 (one-hot);   B = 3, V = 25: an evaluation batch with permuted labels, no gradients
Labels: arange, a permutation of 0..40 that is no involution, and a labels[:41] in which positions 5 and 29 share class 3 and
class 7 is missing -- columns 5 and 29 are then bit-identical and a row whose maximum they are must predict 5.

Bars.
    logits                2e-5 absolute (tests/test_gpu_parity.py);  8-bit logits: 2e-4 against the e4m3 emulation of
                          tests/test_gpu_fp8.py::test_head_logits_on_the_8bit_mfma, everything else of that case against the
                          reference's from-logits entry on the logits the head returned (straight-through)
    loss                  2e-6 relative (global negatives: 3e-6, their table 2e-5 relative: tests/test_gpu_global_batch.py)
    loss_correct[1]       == (pred == labels[:41]).sum(), exactly
    predictions           exact on every row whose float64 top-2 margin exceeds 4e-5 (twice the logits bar); the rows left out may
                          be at most 0.2 % of a case (the reference alone leaves out ~0.04 % with unit-normal inputs)
    d_easy_w, d_easy_b    2e-4 of the tensor's largest entry (test_backward_f32, recompute_check)
    dL/dz, dL/dzg         every row against ITS OWN largest reference entry.  f32: DZ_BAR_F32 = 4 x F32_BASELINE, where
                          F32_BASELINE is the worst row of a plain torch float32 evaluation of the same formulas
                          (head_reference(dtype=torch.float32)) against the float64 reference on this module's inputs, every f32
                          case, measured on the CPU: 9.2e-7 (one-hot, 2049 groups; 3.8e-7 at 1 group,
                          8.2e-7 for dL/dzg at 2049 groups), so DZ_BAR_F32 = 3.7e-6.
                          bf16 (and the 8-bit head, which stores bf16): the f32 bar plus 2^-8 of the reference entry (the
                          kernel computes in f32 and rounds once on store).  Columns 16..63 of every row: exactly 0.
Sensitivity, asserted in every case on the reference alone: the reference's dz with its last row zeroed fails the row-by-row check,
and the loss summed without the last group (still divided by G, as a kernel that skipped its tail group would) misses the loss bar.

Measured on the device (MI355X): worst over the cases of a kind (every case prints its own line)

    kind                              logits   loss rel   dz row    dzg row   d_easy_w  d_easy_b  rows left out
    one-hot f32, 1 .. 2049 groups     3.0e-07  8.4e-08    1.12e-06     -      5.2e-07   7.2e-07   <= 0.057 %
    one-hot f32, V = 3 / V = 25       2.4e-07  5.2e-08    5.2e-07      -      1.4e-07   6.0e-07   0 / 0.195 %
    glove f32, 5 .. 2049              2.9e-07  6.1e-08    8.2e-07   8.7e-07      -         -      <= 0.045 %
    global negatives f32, 5 .. 2049   2.6e-07  7.2e-08    1.02e-06     -      6.0e-07   4.8e-07   <= 0.044 %   (table 2.0e-07)
    bf16, all kinds, 5 .. 8193        as f32   as f32     3.89e-03  3.89e-03  as f32    as f32    as f32       (2^-8 = 3.91e-03)
    8-bit logits, 5 / 2049            6.5e-05  1.0e-07    3.88e-03     -      5.2e-07   4.4e-07   <= 0.036 %
                       bar            2e-5     2e-6       3.7e-06 (+ 2^-8 of the entry in 16-bit storage)  2e-4   0.2 %

The f32 kernel's worst row, 1.12e-06 of the row's largest entry (2049 groups), is 1.2 times the float32 torch baseline.  No
prediction differed on a row with a margin, loss_correct[1] was exact and columns 16..63 were zero in every case; the 8193-group
case (a 4 GB workspace) takes 0.07 s.

What the module found.  The 8-bit head (F8L) formed z_hat . dz_hat, the normalisation backward's projection, as sum_j dl l with
its QUANTISED logits, while dz_hat = dl E_hat is made of the f32 unit vectors: dz kept a component along z, 3.3e-02 (5 groups) and
9.5e-02 (2049 groups) of a row's largest entry against this module's from-logits reference.  head.cuh now takes the projection
from the product itself in that instantiation (3.6e-03 / 3.9e-03: the bf16 store).  And cp_head / cp_head_gneg accepted an n_groups
that is no multiple of V (z rows past n_windows) and a misaligned z; they refuse both now (tests/test_cabi_and_host.py).
"""
import pytest
import torch

from oracle import head_cpu as hc

pytestmark = pytest.mark.gpu

T = 41
LOGITS_BAR, FP8_LOGITS_BAR = 2e-5, 2e-4
LOSS_BAR, GNEG_LOSS_BAR, GNEG_TABLE_BAR = 2e-6, 3e-6, 2e-5
TABLE_GRAD_BAR = 2e-4
MARGIN, EXCLUDED_CAP = 4e-5, 0.002
F32_BASELINE = 9.2e-7
DZ_BAR_F32 = 4 * F32_BASELINE
BF16_STEP = 2.0 ** -8
W_KEY, B_KEY = "glove_net.easy.0.weight", "glove_net.easy.0.bias"
DUP = (5, 29)


def permutation():
    p = torch.randperm(T, generator=torch.Generator().manual_seed(3))
    assert not torch.equal(p[p], torch.arange(T))                 # no involution (so not the identity either)
    return p


def shared_class():
    y = torch.randperm(T, generator=torch.Generator().manual_seed(4))
    y[(y == 3).nonzero()[0, 0]], y[(y == 7).nonzero()[0, 0]] = y[DUP[0]].item(), y[DUP[1]].item()
    y[DUP[0]], y[DUP[1]] = 3, 3
    assert sorted(set(range(T)) - set(y.tolist())) == [7] and (y == 3).nonzero().flatten().tolist() == list(DUP)
    return y


LAYOUTS = {"arange": lambda: torch.arange(T), "perm": permutation, "shared": shared_class}


class Case:
    def __init__(self, variant, dtype, groups, V=1, layout="arange", want_grad=True):
        self.variant, self.dtype, self.groups, self.V, self.layout, self.want_grad = variant, dtype, groups, V, layout, want_grad
        self.id = f"{variant}-{dtype}-{groups}" + (f"x{V}" if V > 1 else "") + ("" if layout == "arange" else "-" + layout) + \
                  ("" if want_grad else "-nograd")

    def inputs(self):
        """CPU f32 tensors; the seed is a function of the shape alone, so the variants of one shape see the same z"""
        G, V = self.groups, self.V
        assert G % V == 0
        B, n = G // V, G * T
        g = torch.Generator().manual_seed(1000 + 7 * G + V)
        z = torch.randn(n, 16, generator=g) * 10.0 ** (6 * torch.rand(n, 1, generator=g) - 3)
        w = torch.randn(16, T, generator=g) * (0.5 + 1.5 * torch.rand(1, T, generator=g))
        b = 0.3 * torch.randn(16, generator=g)
        zg = torch.randn(B * T, 16, generator=g) * 10.0 ** (4 * torch.rand(B * T, 1, generator=g) - 2)
        y = LAYOUTS[self.layout]()
        if self.layout == "shared":
            # four rows of every group point at the shared class (within noise), so that the tied columns ARE row maxima
            E = (w.t() + b[None])[3]
            zv = z.reshape(B, T, V, 16)
            for i in (0, DUP[0], 17, DUP[1]):
                zv[:, i] = (E[None, None] + 0.1 * torch.randn(B, V, 16, generator=g)) * zv[:, i].norm(dim=-1, keepdim=True)
        return dict(z=z, w=w, b=b, zg=zg, labels=y.repeat(B))


CASES = ([Case("onehot", "f32", G) for G in (1, 5, 256, 257, 2047, 2048, 2049)] +
         [Case("onehot", "f32", G, layout=lay) for G in (5, 257) for lay in ("perm", "shared")] +
         [Case("onehot", "bf16", G) for G in (5, 257, 2049, 8193)] +
         [Case("glove", dt, G) for dt in ("f32", "bf16") for G in (5, 257, 2049)] +
         [Case("glove", "f32", G, layout="perm") for G in (5, 257)] +
         [Case("gneg", dt, G) for dt in ("f32", "bf16") for G in (5, 257, 2049)] +
         [Case("fp8", "fp8", G) for G in (5, 2049)] +
         [Case("onehot", dt, 6, V=3, layout="perm") for dt in ("f32", "bf16")] +
         [Case("onehot", "f32", 75, V=25, layout="perm", want_grad=False)])

_engines = {}


def engine(dtype, class_encoder):
    from contrastiveprosthetics_amd.engine import Engine
    key = (dtype, class_encoder)
    if key not in _engines:
        _engines[key] = Engine(adabn=True, dtype=dtype, device="cuda", class_encoder=class_encoder)
    return _engines[key]


def run_head(case, inp):
    """the head on its own: poisoned workspaces and gradient store, one call, everything it left behind"""
    from contrastiveprosthetics_amd import _lib
    glove = case.variant == "glove"
    e = engine(case.dtype, "glove" if glove else "onehot")
    z, labels = inp["z"].cuda(), inp["labels"].cuda()
    n = z.shape[0]
    e.values.views[W_KEY].copy_(inp["w"])
    e.values.views[B_KEY].copy_(inp["b"])
    e.grads.flat.fill_(float("nan"))
    e.workspace(n)[(_lib.FP8_STATE_BYTES if case.dtype == "fp8" else 0):].fill_(0xFF)
    got = {}
    if glove:
        zg = inp["zg"].cuda()
        e._gws_args(zg.shape[0])
        e._gws.fill_(0xFF)
        out, pred, logits = e.head_glove(z, zg, labels, case.V, want_grad=case.want_grad, want_logits=True)
    else:
        gh = None
        if case.variant == "gneg":
            gh = got["gh"] = e.global_negatives(z, labels)
        out, pred, logits = e.head(z, labels, case.V, want_grad=case.want_grad, want_logits=True, gneg=gh)
    got.update(loss=out[0], correct=out[1], pred=pred, logits=logits)
    if case.want_grad:
        got["dz"] = e.debug_head_grad()
        if glove:
            got["dzg"] = e.debug_glove_head_grad()
        else:
            got["d_easy_w"], got["d_easy_b"] = e.grads.views[W_KEY].clone(), e.grads.views[B_KEY].clone()
    torch.cuda.synchronize()
    return got


def rows_within(got, ref, dtype):
    """(every row within its bar, worst row error over that row's largest reference entry); NaN fails"""
    got, rowmax = got.double(), ref.abs().max(dim=1, keepdim=True).values
    err = (got - ref).abs()
    allowed = DZ_BAR_F32 * rowmax + (0.0 if dtype == "f32" else BF16_STEP) * ref.abs()
    return bool((err <= allowed).all()), float((err / rowmax).max())


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_head_against_float64(case):
    inp = case.inputs()
    got = run_head(case, inp)
    dev = {k: v.cuda() for k, v in inp.items()}
    G, V, y = case.groups, case.V, dev["labels"][:T]
    cls = dict(zg=dev["zg"]) if case.variant == "glove" else dict(easy_w=dev["w"], easy_b=dev["b"])
    table = got["gh"].double() if case.variant == "gneg" else None
    true = hc.head_reference(dev["z"], dev["labels"], V, gneg=table, want_grad=case.want_grad, **cls)
    fig, fails = {}, []                     # every figure is printed before anything is asserted

    def bar(name, value, limit):
        fig[name] = value
        if not value <= limit:              # (NaN fails)
            fails.append(f"{name} {value:.3e} > {limit:.1e}")

    # ---- logits
    if case.variant == "fp8":
        zh = dev["z"] / dev["z"].norm(dim=-1, keepdim=True)
        E = dev["w"].t() + dev["b"][None]
        q = lambda t: t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32)
        emu = q(zh).reshape(G, T, 16) @ q(E / E.norm(dim=-1, keepdim=True)).t()[None]
        bar("logits", float((got["logits"] - emu).abs().max()), FP8_LOGITS_BAR)
        ref = hc.head_from_logits(got["logits"], dev["z"], dev["labels"], V, **cls)
    else:
        bar("logits", float((got["logits"].double() - true["logits"]).abs().max()), LOGITS_BAR)
        ref = true

    # ---- loss; a tail group left out of the sum (still divided by G) could not pass
    loss_bar = GNEG_LOSS_BAR if case.variant == "gneg" else LOSS_BAR
    bar("loss rel", abs(float(got["loss"]) - float(ref["loss"])) / float(ref["loss"]), loss_bar)
    per_group = hc.loss_per_group(ref["logits"], dev["labels"], table)
    assert abs(float(per_group.mean()) - float(ref["loss"])) <= 1e-12 * float(ref["loss"])
    without_last = float(per_group[:-1].sum()) / G
    assert abs(without_last - float(ref["loss"])) / float(ref["loss"]) > loss_bar, "a skipped last group would pass the loss bar"

    # ---- predictions, first maximum
    lo = ref["logits"]
    if case.layout == "shared":
        lo = lo.clone()
        lo[:, :, DUP[1]] = -float("inf")                                                    # (the margin of a tied pair is its gap to the rest)
    top2 = lo.topk(2, dim=-1).values
    keep = (top2[..., 0] - top2[..., 1]) > MARGIN
    bar("excluded rows", 1.0 - float(keep.double().mean()), EXCLUDED_CAP)
    bar("wrong predictions", float((got["pred"][keep].long() != ref["pred"][keep]).sum()), 0)
    bar("correct count off by", abs(float(got["correct"]) - float((got["pred"] == y[None]).sum())), 0)
    if case.layout == "shared":
        tied = keep & (ref["pred"] == DUP[0])                                               # the rows aimed at the shared class
        assert int(tied.sum()) >= 2 * G
        bar("tied columns differ", float((got["logits"][:, :, DUP[0]] != got["logits"][:, :, DUP[1]]).sum()), 0)
        bar("ties to the upper column", float((got["pred"] == DUP[1]).sum() + (got["pred"][tied] != DUP[0]).sum()), 0)

    if case.variant == "gneg":
        own = hc.gneg_table(true["logits"], dev["labels"])
        bar("table rel", float(((got["gh"][:, :T].double() - own).abs() / own.abs()).max()), GNEG_TABLE_BAR)
    if case.want_grad:
        for k in ("dz", "dzg") if case.variant == "glove" else ("dz",):
            assert got[k].shape == (ref[k].shape[0], 64)
            bar(k + " cols 16..63 non-zero", float((got[k][:, 16:] != 0).sum()), 0)
            ok, worst = rows_within(got[k][:, :16], ref[k], case.dtype)
            fig[k + " row"] = worst
            if not ok:
                fails.append(f"{k}: worst row error {worst:.3e} of the row's largest entry (f32 bar {DZ_BAR_F32:.1e}"
                             + ("" if case.dtype == "f32" else " + 2^-8 of the entry") + ")")
            skipped = ref[k].clone()
            skipped[-1] = 0
            assert not rows_within(skipped, ref[k], case.dtype)[0], f"{k}: a skipped last row would pass"
        if case.variant != "glove":
            for k in ("d_easy_w", "d_easy_b"):
                bar(k, float((got[k].double() - ref[k]).abs().max()) / float(ref[k].abs().max()), TABLE_GRAD_BAR)
    print(f"\nhead {case.id:26s} G {G:5d} V {V:2d} | " + "  ".join(
        f"{k} {100 * v:.3f} %" if k == "excluded rows" else f"{k} {v:.2e}" for k, v in fig.items() if v != 0 or k in ("logits", "loss rel", "excluded rows")))
    assert not fails, "; ".join(fails)
