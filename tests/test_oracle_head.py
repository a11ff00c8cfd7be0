"""oracle/head_cpu.py, the float64 reference that tests/test_gpu_head.py holds csrc/head.cuh against, is itself held against the
oracle's statement of the reference (oracle/ref_cpu.py: OracleModel.loss, the per-group loop of code/models.py:132-173, 198-208,
and its one-shot forms) and its gradients against central differences.  CPU only."""
import pytest
import torch

from oracle import head_cpu as hc
from oracle import ref_cpu as oc

T = oc.N_TASKS
PARAMS = dict(reg_emg=0.0, reg_glove=0.0)


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def permutation(seed=3):
    p = torch.randperm(T, generator=torch.Generator().manual_seed(seed))
    assert not torch.equal(p[p], torch.arange(T)) and not torch.equal(p, torch.arange(T))       # not an involution
    return p


def shared_class():
    """positions 5 and 29 both carry class 3; class 7 is missing (not the largest: F.one_hot sizes the table by the maximum)"""
    y = permutation(4).clone()
    y[(y == 3).nonzero()[0, 0]], y[(y == 7).nonzero()[0, 0]] = y[5].item(), y[29].item()
    y[5], y[29] = 3, 3
    assert sorted(set(range(T)) - set(y.tolist())) == [7] and int((y == 3).sum()) == 2
    return y


def oracle_model(seed, training):
    sd = {k: v.double() if v.dtype.is_floating_point else v for k, v in oc.init_state_dict(seed, 16, True).items()}
    sd["glove_net.easy.0.bias"] = 0.3 * randn(seed + 50, 16)
    m = oc.OracleModel(sd, PARAMS, adabn=True)
    m.training = training
    return m, sd["glove_net.easy.0.weight"], sd["glove_net.easy.0.bias"]


def oracle_logits(m, z, labels, B, V):
    """Model.forward from the encoder's output on (models.py:121-130), with the oracle's own class encoder and regroup"""
    ze = z.reshape(B, T, V, 16).transpose(1, 2).reshape(-1, T, 16)
    ze = ze / ze.norm(dim=-1, keepdim=True)
    zc = m.encode_class(torch.zeros(B, T, oc.GLOVE_DIM), labels)
    zc = zc / zc.norm(dim=-1, keepdim=True)
    m.shape = (B, T, V, 1, 12)
    return torch.bmm(ze, zc.transpose(1, 2))


def loop_f64(logits, labels, times):
    """the per-group loop of code/models.py:132-147, 198-208 with a float64 accumulator (OracleModel._loopy adds into a float32
    torch.zeros(1), as the reference does: it pins the value to 1e-6, this loop to rounding)"""
    G = logits.shape[0] // times
    tgt = torch.cat([labels[:T]] * times)
    le = sum(torch.nn.functional.cross_entropy(log.reshape(-1, T), tgt) for log in logits.reshape(G, times, T, T)) / G
    lg = sum(torch.nn.functional.cross_entropy(log.reshape(-1, T), tgt) for log in logits.transpose(1, 2).reshape(G, times, T, T)) / G
    return (le + lg) / 2


def test_equals_the_one_shot_forms_at_arange_labels():
    B = 3
    m, w, b = oracle_model(1, True)
    z, labels = randn(2, B * T, 16), torch.arange(T).repeat(B)
    lo = oracle_logits(m, z, labels, B, 1)
    r = hc.head_reference(z, labels, 1, w, b)
    assert float((r["logits"] - lo).abs().max()) < 1e-14
    assert abs(float(r["loss"]) - float(m.loss_vectorized(lo, labels))) < 1e-13
    assert abs(float(r["loss"]) - float(m.loss(lo, labels))) < 1e-6
    assert abs(float(r["loss"]) - float(loop_f64(lo, labels, 1))) < 1e-13
    assert int(r["correct"]) == round(m.corrects[-1] * B * T)
    g = hc.head_reference(z, labels, 1, w, b, gneg=True)
    assert abs(float(g["loss"]) - float(m.loss_global_negatives(lo, labels))) < 1e-13
    assert torch.equal(g["logits"], r["logits"]) and g["gh"].shape == (2, T)
    # one group: the extension is the reference's loss
    one = hc.head_reference(z[:T], labels[:T], 1, w, b, gneg=True)
    assert abs(float(one["loss"]) - float(hc.head_reference(z[:T], labels[:T], 1, w, b)["loss"])) < 1e-13


@pytest.mark.parametrize("layout", ["permutation", "shared_class"])
@pytest.mark.parametrize("V", [1, oc.VOTE_SAMPLES])
def test_equals_the_per_group_loop_at_other_labels(layout, V):
    B = 2
    y = permutation() if layout == "permutation" else shared_class()
    m, w, b = oracle_model(5, training=(V == 1))
    z, labels = randn(6, B * T * V, 16), y.repeat(B)
    lo = oracle_logits(m, z, labels, B, V)
    r = hc.head_reference(z, labels, V, w, b)
    assert r["logits"].shape == (B * V, T, T) and float((r["logits"] - lo).abs().max()) < 1e-14
    assert abs(float(r["loss"]) - float(m.loss(lo, labels))) < 1e-6
    assert abs(float(r["loss"]) - float(loop_f64(lo, labels, V))) < 1e-13
    assert torch.equal(r["pred"], lo.argmax(-1))
    if V == 1:
        assert int(r["correct"]) == round(m.corrects[-1] * B * T)
    if layout == "shared_class":
        assert torch.equal(r["logits"][:, :, 5], r["logits"][:, :, 29])                   # bit-identical columns
        assert not bool((r["pred"] == 29).any())                                          # first maximum: the lower column


def central_differences(f, x, picks, h=1e-6):
    out = []
    for i in picks:
        d = torch.zeros_like(x).flatten()
        d[i] = h
        d = d.reshape(x.shape)
        out.append((float(f(x + d)) - float(f(x - d))) / (2 * h))
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("variant", ["onehot", "onehot_v3", "shared_class", "glove", "gneg", "gneg_table"])
def test_gradients_match_central_differences(variant):
    B, V = 2, (3 if variant == "onehot_v3" else 1)
    y = dict(shared_class=shared_class(), onehot_v3=permutation()).get(variant, torch.arange(T))
    labels = y.repeat(B)
    z = randn(11, B * T * V, 16) * torch.logspace(-1, 1, B * T * V, dtype=torch.float64)[:, None]
    w, b, zg = randn(12, 16, T), 0.3 * randn(13, 16), randn(14, B * T, 16)
    kw = dict(zg=zg) if variant == "glove" else dict(easy_w=w, easy_b=b)
    gneg = True if variant.startswith("gneg") else None
    r = hc.head_reference(z, labels, V, gneg=gneg, **kw)
    if variant == "gneg_table":
        # the table as an input (what the kernel sees): same loss, same gradients as differentiating through G
        t = hc.head_reference(z, labels, V, gneg=torch.cat([r["gh"], torch.zeros(2, 23, dtype=torch.float64)], 1), **kw)
        assert abs(float(t["loss"]) - float(r["loss"])) < 1e-14
        for k in ("dz", "d_easy_w", "d_easy_b"):
            assert float((t[k] - r[k]).abs().max()) < 1e-13 * float(r[k].abs().max()), k
        return
    g = torch.Generator().manual_seed(15)
    for name, x, key in (("z", z, "dz"),) + ((("zg", zg, "dzg"),) if variant == "glove" else
                                             (("easy_w", w, "d_easy_w"), ("easy_b", b, "d_easy_b"))):
        picks = torch.randperm(x.numel(), generator=g)[:16].tolist()
        kw2 = dict(kw)

        def f(v, name=name):
            a = dict(kw2)
            if name != "z":
                a[name] = v
            return hc.head_reference(v if name == "z" else z, labels, V, gneg=gneg, want_grad=False, **a)["loss"]
        h = 1e-5 * float(x.flatten()[picks].abs().max().clamp(min=1.0))
        fd = central_differences(f, x, picks, h)
        an = r[key].flatten()[picks]
        # (the difference quotient's own rounding: the loss, ~3.7, to 2^-52 over 2h)
        floor = 8 * 2.0 ** -52 * float(r["loss"]) / h
        assert float((fd - an).abs().max()) < 1e-6 * float(r[key].abs().max()) + floor, (variant, name, fd, an)


def test_from_logits_entry_is_straight_through():
    """at the true logits the second entry IS the first; at perturbed logits its loss, predictions and dl follow the logits given
    while the two products keep the unquantised unit vectors: dz stays orthogonal to z, and equals the explicit formula"""
    B, V = 2, 1
    labels = permutation().repeat(B)
    z, w, b = randn(21, B * T, 16) * 3.0, randn(22, 16, T), 0.3 * randn(23, 16)
    r = hc.head_reference(z, labels, V, w, b)
    s = hc.head_from_logits(r["logits"], z, labels, V, w, b)
    for k in ("loss", "dz", "d_easy_w", "d_easy_b"):
        assert float((s[k] - r[k]).abs().max()) < 1e-14, k
    assert torch.equal(s["pred"], r["pred"])
    q = r["logits"] + 0.02 * randn(24, B, T, T)
    s = hc.head_from_logits(q, z, labels, V, w, b)
    assert abs(float(s["loss"]) - float(hc.loss_of_logits(q, labels))) < 1e-15 and torch.equal(s["pred"], q.argmax(-1))
    zh = z / z.norm(dim=-1, keepdim=True)
    E = hc.class_rows(w, b)
    eh = (E / E.norm(dim=-1, keepdim=True))[labels].reshape(B, T, 16)
    dzh = torch.bmm(s["dl"], eh).reshape(-1, 16)
    want = (dzh - zh * (zh * dzh).sum(-1, keepdim=True)) / z.norm(dim=-1, keepdim=True)
    assert float((s["dz"] - want).abs().max()) < 1e-14
    assert float((s["dz"] * z).sum(-1).abs().max()) < 1e-15
