"""The float64 reference of tests/test_gpu_head_temperature.py (tests/head_temperature_ref.py: torch autograd over
exp(clamp(s)) * oracle.head_cpu.head_logits fed to oracle.head_cpu.loss_of_logits) anchored on the CPU: at s = 0 it is
oracle.head_cpu.head_reference, its dL/ds is sum dl * logits and a central finite difference of the loss, and 0 outside
[-ln 100, ln 100]; the straight-through form agrees with it on unquantised logits; and the cases of the GPU module leave out at
most 0.2 % of their rows by the cosine-margin rule (the cap the reference alone must meet)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_temperature_ref as tr  # noqa: E402  (tests/head_temperature_ref.py)
from oracle import head_cpu as hc  # noqa: E402

T = 41


def inputs(G, V=1, seed=5, perm=False):
    g = torch.Generator().manual_seed(seed)
    n = G * T
    z = torch.randn(n, 16, generator=g) * 10.0 ** (6 * torch.rand(n, 1, generator=g) - 3)
    w = torch.randn(16, T, generator=g) * (0.5 + 1.5 * torch.rand(1, T, generator=g))
    b = 0.3 * torch.randn(16, generator=g)
    zg = torch.randn(G // V * T, 16, generator=g)
    y = torch.randperm(T, generator=torch.Generator().manual_seed(3)) if perm else torch.arange(T)
    return z, w, b, zg, y.repeat(G // V)


@pytest.mark.parametrize("glove,G,V,perm", [(False, 3, 1, False), (False, 6, 3, True), (True, 3, 1, False), (True, 5, 1, True)])
def test_equals_head_reference_at_zero(glove, G, V, perm):
    z, w, b, zg, labels = inputs(G, V, perm=perm)
    cls = dict(zg=zg) if glove else dict(easy_w=w, easy_b=b)
    a, r = tr.temp_reference(z, labels, V, 0.0, **cls), hc.head_reference(z, labels, V, **cls)
    for k in ("logits", "loss", "dz") + (("dzg",) if glove else ("d_easy_w", "d_easy_b")):
        assert float((a[k] - r[k]).abs().max()) <= 1e-12 * max(1.0, float(r[k].abs().max())), k
    assert torch.equal(a["pred"], r["pred"]) and int(a["correct"]) == int(r["correct"])
    assert torch.equal(a["logits"], a["cosines"])


@pytest.mark.parametrize("s", [math.log(0.5), math.log(1 / 0.07), tr.S_MAX_F32, -tr.S_MAX_F32, 1.0])
def test_ds_is_sum_dl_l_and_a_finite_difference(s):
    z, w, b, zg, labels = inputs(4)
    r = tr.temp_reference(z, labels, 1, s, easy_w=w, easy_b=b)
    assert float(r["ds"]) == pytest.approx(float(r["dl_l"].sum()), rel=1e-12, abs=1e-15)
    assert float(r["abs_dl_l"]) >= abs(float(r["ds"]))
    h = 1e-6
    # (at the bound itself the clamp has a one-sided derivative: step inwards on both sides of a point just inside)
    c = s - 2 * h if s > 4 else s + 2 * h if s < -4 else s
    rc = tr.temp_reference(z, labels, 1, c, easy_w=w, easy_b=b)
    up = tr.temp_reference(z, labels, 1, c + h, easy_w=w, easy_b=b, want_grad=False)["loss"]
    dn = tr.temp_reference(z, labels, 1, c - h, easy_w=w, easy_b=b, want_grad=False)["loss"]
    assert float((up - dn) / (2 * h)) == pytest.approx(float(rc["ds"]), rel=1e-6, abs=1e-9)
    # the data gradients carry tau: dz = tau * (dz of the cosines' loss at the same dl)
    assert abs(float(r["ds"])) > 0


@pytest.mark.parametrize("s", [5.0, -5.0, tr.S_MAX + 1e-9, float(torch.tensor(tr.S_MAX, dtype=torch.float32))])
def test_zero_outside_the_clamp(s):
    z, w, b, zg, labels = inputs(3)
    r = tr.temp_reference(z, labels, 1, s, easy_w=w, easy_b=b)
    edge = tr.temp_reference(z, labels, 1, math.copysign(tr.S_MAX, s), easy_w=w, easy_b=b)
    assert float(r["ds"]) == 0.0
    assert float((r["logits"] - edge["logits"]).abs().max()) <= 1e-12 * 100 and float(r["loss"]) == pytest.approx(float(edge["loss"]), rel=1e-13)
    assert abs(float(edge["ds"])) > 0 and float(edge["dl_l"].sum()) == pytest.approx(float(r["dl_l"].sum()), rel=1e-9)


def test_bound_as_a_float32():
    import numpy as np
    assert np.float32(tr.S_MAX_F32) == tr.S_MAX_F32 <= tr.S_MAX < float(np.nextafter(np.float32(tr.S_MAX_F32), np.float32(10)))
    assert tr.SCALES["ln 100"] == tr.S_MAX_F32 and tr.tau_of(5.0) == pytest.approx(100.0, rel=1e-15)
    from contrastiveprosthetics_amd.engine import LOGIT_SCALE_MAX
    assert LOGIT_SCALE_MAX == tr.S_MAX_F32


def test_straight_through_form_on_unquantised_logits():
    z, w, b, zg, labels = inputs(3)
    for s in (math.log(1 / 0.07), 5.0):
        r = tr.temp_reference(z, labels, 1, s, easy_w=w, easy_b=b)
        f = tr.temp_from_logits(r["logits"], z, labels, 1, s, w, b)
        for k in ("loss", "dz", "d_easy_w", "d_easy_b", "ds", "dl_l", "abs_dl_l"):
            assert float((f[k] - r[k]).abs().max()) <= 1e-12 * max(1.0, float(r[k].abs().max())), (k, s)


def test_param_table_with_a_learnt_temperature():
    from contrastiveprosthetics_amd.engine import FlatStore, l2_member, param_specs
    for enc in ("onehot", "glove"):
        plain, temp = param_specs(True, 16, enc), param_specs(True, 16, enc, logit_scale=True)
        assert list(temp)[:-1] == list(plain) and list(temp)[-1] == "logit_scale" and temp["logit_scale"] == ()
        a, b = FlatStore(plain, "cpu"), FlatStore(temp, "cpu")
        assert all(b.offsets[k] == a.offsets[k] for k in plain)           # trailing: every existing offset unchanged
        assert b.offsets["logit_scale"][1] == 1 and b.views["logit_scale"].shape == ()
        assert not l2_member("logit_scale")


def test_gpu_cases_meet_the_excluded_rows_cap():
    """the rows the GPU module leaves out of the prediction check (float64 cosine top-2 margin <= 4e-5): at most 0.2 % of a case"""
    import test_gpu_head_temperature as tg
    worst = {}
    for case in tg.CASES:
        if case.variant == "fp8":
            continue                                                       # (its margins are those of the logits the device returns)
        inp = case.inputs()
        cls = dict(zg=inp["zg"]) if case.variant == "glove" else dict(easy_w=inp["w"], easy_b=inp["b"])
        cos = hc.head_logits(inp["z"].double(), inp["labels"], case.V, **{k: v.double() for k, v in cls.items()})
        top2 = cos.topk(2, dim=-1).values
        worst[case.id] = 1.0 - float(((top2[..., 0] - top2[..., 1]) > tg.MARGIN).double().mean())
    print({k: f"{100 * v:.3f} %" for k, v in worst.items()})
    assert max(worst.values()) <= tg.EXCLUDED_CAP, worst
