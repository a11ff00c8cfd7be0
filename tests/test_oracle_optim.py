"""oracle/optim_cpu.py, the float64 reference that tests/test_gpu_optim.py holds csrc/optim.cuh against, is itself held against
what the reference program runs: two torch.optim.Adam with their own learning rates (oracle/ref_cpu.py::make_optimizers,
code/train.py:72-73) stepping on the data gradient plus autograd of reg * sum(torch.norm(t)) over the members
(code/models.py:344-349, 467-472), in float64.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import optim_cpu as oc

#          offset, numel, group, l2      (gaps between the tensors; ragged sizes; the four group / l2 combinations)
TABLE = [(3, 5, 0, 1),
         (9, 1, 1, 1),
         (12, 7, 1, 0),
         (20, 6, 0, 1),                  # all zero: a member without a norm
         (27, 4, 0, 0),                  # no member, zero gradient, zero moments: must not move
         (31, 0, 1, 1),                  # no element
         (33, 11, 1, 1)]
LENGTH = 47
ZERO_MEMBER, STILL = 3, 4
HYPER = dict(lr_emg=1e-3, lr_glove=3e-2, reg_emg=1e-3, reg_glove=2e-2, beta1=0.9, beta2=0.999, eps=1e-8)
REL = 1e-12


def randn(seed, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def start():
    p, m = randn(1, LENGTH), 1e-2 * randn(2, LENGTH)
    v = m * m
    off, n = TABLE[ZERO_MEMBER][:2]
    p[off:off + n] = 0
    off, n = TABLE[STILL][:2]
    m[off:off + n] = 0
    v[off:off + n] = 0
    return p, m, v


def gradient(step):
    g = randn(10 + step, LENGTH) * 10.0 ** (2 * torch.rand(LENGTH, generator=torch.Generator().manual_seed(20 + step), dtype=torch.float64) - 2)
    off, n = TABLE[STILL][:2]
    g[off:off + n] = 0
    return g


def close(a, b):
    return bool(((a - b).abs() <= REL * b.abs()).all())


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_reference_equals_two_torch_adams_with_autograd_of_the_norms(grad_scale):
    h = {k: oc.as_float32(x) for k, x in HYPER.items()}          # the reference takes the float32 values: so must the optimisers
    p0, m, v = start()
    leaves = [p0[o:o + n].clone().requires_grad_(True) for o, n, _, _ in TABLE]
    opts = [torch.optim.Adam([t for t, row in zip(leaves, TABLE) if row[2] == grp], lr=h["lr_" + name], betas=(h["beta1"], h["beta2"]),
                             eps=h["eps"], weight_decay=0) for grp, name in ((0, "emg"), (1, "glove"))]
    # the moments the first step starts from, as torch.optim.Adam keeps them (its step counter starts at 0)
    for o in opts:
        for t in o.param_groups[0]["params"]:
            i = next(k for k, x in enumerate(leaves) if x is t)
            off, n = TABLE[i][:2]
            o.state[t] = dict(step=torch.tensor(0.0), exp_avg=m[off:off + n].clone(), exp_avg_sq=v[off:off + n].clone())
    p = p0.clone()
    for step in (1, 2, 3):
        g = gradient(step)
        # torch.optim.Adam keeps its bias corrections in double: the reference is given those (the float32 rounding of the
        # library's host code, which `step=` applies, is pinned in the next test)
        ref = oc.l2_adam_reference(p, g, m, v, TABLE, HYPER, grad_scale=grad_scale, bc1=1.0 - h["beta1"] ** step,
                                   bc2=1.0 - h["beta2"] ** step)
        for o in opts:
            o.zero_grad(set_to_none=True)
        norms = [torch.norm(t) for t in leaves]
        value = sum(h["reg_glove" if row[2] else "reg_emg"] * n for n, row in zip(norms, TABLE) if row[3])
        value.backward()                                          # torch.norm's gradient at the zero tensor is 0
        for t, (off, n, _, _) in zip(leaves, TABLE):
            data = oc.as_float32(grad_scale) * g[off:off + n]
            t.grad = data if t.grad is None else t.grad + data
        for o in opts:
            o.step()
        assert abs(float(ref["l2"]) - float(value.detach())) <= REL * float(value.detach())
        for i, (t, (off, n, grp, l2)) in enumerate(zip(leaves, TABLE)):
            o = opts[grp]
            assert abs(float(ref["norms"][i]) - float(norms[i].detach())) <= REL * float(norms[i].detach())
            assert close(ref["p"][off:off + n], t.detach()), (step, i)
            assert close(ref["m"][off:off + n], o.state[t]["exp_avg"]), (step, i)
            assert close(ref["v"][off:off + n], o.state[t]["exp_avg_sq"]), (step, i)
        # outside the table nothing moves
        inside = torch.zeros(LENGTH, dtype=torch.bool)
        for off, n, _, _ in TABLE:
            inside[off:off + n] = True
        for k, was in (("p", p), ("m", m), ("v", v)):
            assert torch.equal(ref[k][~inside], was[~inside])
        # the member without a norm follows its data gradient and stays finite; the still tensor is bit-identical
        off, n = TABLE[ZERO_MEMBER][:2]
        assert bool(torch.isfinite(ref["p"][off:off + n]).all()) and bool((ref["p"][off:off + n] != 0).all())
        assert float(ref["norms"][ZERO_MEMBER]) == 0.0 if step == 1 else float(ref["norms"][ZERO_MEMBER]) > 0
        off, n = TABLE[STILL][:2]
        assert torch.equal(ref["p"][off:off + n], p0[off:off + n])
        assert not bool(ref["m"][off:off + n].any()) and not bool(ref["v"][off:off + n].any())
        assert not bool(ref["m_scale"][off:off + n].any()) and not bool(ref["p_scale"][off:off + n].any())
        p, m, v = ref["p"], ref["m"], ref["v"]


def test_bias_corrections_are_the_host_codes_float32_values():
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    for t in (1, 2, 3, 1000):
        bc1, bc2 = oc.bias_corrections(0.9, 0.999, t)
        assert bc1 == float(np.float32(1.0 - b1 ** t)) and bc2 == float(np.float32(1.0 - b2 ** t))
        assert bc1 == float(np.float32(bc1)) and bc2 == float(np.float32(bc2))
    p, m, v = start()
    g = gradient(1)
    a = oc.l2_adam_reference(p, g, m, v, TABLE, HYPER, step=3)
    bc1, bc2 = oc.bias_corrections(0.9, 0.999, 3)
    b = oc.l2_adam_reference(p, g, m, v, TABLE, HYPER, bc1=bc1, bc2=bc2, lr_emg=oc.as_float32(HYPER["lr_emg"]),
                                lr_glove=oc.as_float32(HYPER["lr_glove"]))
    for k in ("p", "m", "v", "l2", "norms"):
        assert torch.equal(a[k], b[k]), k


def test_float32_mode_is_the_same_formulas_in_single_precision():
    p, m, v = start()
    g = gradient(1)
    f32 = lambda t: t.float().double()                           # inputs a float32 evaluation can hold
    p, g, m, v = f32(p), f32(g), f32(m), f32(m).pow(2).float().double()
    a = oc.l2_adam_reference(p, g, m, v, TABLE, HYPER, step=1)
    b = oc.l2_adam_reference(p, g, m, v, TABLE, HYPER, step=1, dtype=torch.float32)
    assert b["p"].dtype == torch.float32 and b["l2"].dtype == torch.float32
    inside = a["p_scale"] > 0
    assert float(((b["m"].double() - a["m"]).abs()[inside] / a["m_scale"][inside]).max()) < 1e-6
    # the update to 1e-6 of its natural size, behind the one rounding of the stored parameter
    excess = ((b["p"].double() - a["p"]).abs() - 2.0 ** -24 * a["p"].abs()).clamp(min=0)
    assert float((excess[inside] / a["p_scale"][inside]).max()) < 1e-6
    assert abs(float(b["l2"]) - float(a["l2"])) < 1e-6 * float(a["l2"])
    # a norm given is the norm used
    n = [float(x) for x in a["norms"]]
    n[0] *= 2
    c = oc.l2_adam_reference(p, g, m, v, TABLE, HYPER, step=1, norms=n)
    off, k = TABLE[0][:2]
    assert not torch.equal(c["m"][off:off + k], a["m"][off:off + k]) and torch.equal(c["m"][off + k:], a["m"][off + k:])
