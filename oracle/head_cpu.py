"""The contrastive head on its own, in torch float64 (CPU or device): what csrc/head.cuh computes from z, a class table and
labels, with the semantics of code/models.py:121-173, 198-208 for ANY labels[:41] -- a permutation, or positions that share
a class.

    z       (n, 16), n = B*41*V, window order (b, t, v)            (EMGNet.forward's rows before the regroup of models.py:337-341)
    class rows of group g = b*V + v, position j:
        one-hot   E[labels[b*41 + j]],  E[c] = easy_w[:, c] + easy_b                    (models.py:457-458)
        glove     zg[b*41 + j]                                                          (per-group rows)
    logits[g, i, j] = z_hat[g, i] . e_hat[g, j]                                         (models.py:123-129)
    loss    = (CE(logits[g], y) + CE(logits[g]^T, y)) / 2, meaned over groups, y = labels[:41] for EVERY group   (models.py:147, 204-207)
    pred    = first maximum of every row; correct = number of rows with pred == y       (models.py:149, 165)

Gradients are float64 autograd of that loss: dL/dz in z's own row order, and d_easy_w / d_easy_b or dL/dzg.

head_from_logits is the second entry, for the 8-bit head: loss, predictions and dL/dlogits come from the logits AS GIVEN (the
kernel's quantised ones), the two gradient products dl E_hat and dl^T z_hat use the unquantised unit vectors, and the
normalisations are differentiated exactly -- the kernel's straight-through rule.

global negatives (an extension; identity layout labels[t] = t only): `gneg=True` treats the rows of this call as the
global batch and differentiates through G; `gneg=<(2, >=41) table {G, H}>` takes the table as given, as the kernel does, and
carries the gradient into the negatives through H.  Both return the table they used.
"""
from typing import Dict, Optional, Union

import torch
import torch.nn.functional as F

T = 41
D = 16


def _groups(z: torch.Tensor, V: int) -> torch.Tensor:
    n = z.shape[0]
    assert n % (T * V) == 0 and z.shape[1] == D
    B = n // (T * V)
    return z.reshape(B, T, V, D).transpose(1, 2).reshape(B * V, T, D)


def _unit(x: torch.Tensor) -> torch.Tensor:
    return x / x.norm(dim=-1, keepdim=True)


def class_rows(easy_w: torch.Tensor, easy_b: torch.Tensor) -> torch.Tensor:
    """E (41, 16): E[c] = easy_w[:, c] + easy_b"""
    return easy_w.t() + easy_b[None]


def head_logits(z, labels, V, easy_w=None, easy_b=None, zg=None) -> torch.Tensor:
    """(G, 41, 41) in the dtype of z.  One-hot: the product against the 41 CLASS rows, then a gather by labels, so that
    positions that share a class have bit-identical columns."""
    zh = _unit(_groups(z, V))
    G = zh.shape[0]
    B = G // V
    if zg is not None:
        eh = _unit(zg.reshape(B, 1, T, D)).expand(B, V, T, D).reshape(G, T, D)
        return torch.bmm(zh, eh.transpose(1, 2))
    s = zh @ _unit(class_rows(easy_w, easy_b)).t()                                # (G, 41 rows, 41 classes)
    idx = labels.reshape(B, T).repeat_interleave(V, dim=0)                        # class of position j of group g
    return torch.gather(s, 2, idx[:, None, :].expand(G, T, T))


def gneg_table(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """{G, H} (2, 41) of the rows of `logits` taken as the global batch (identity layout):
    G[k] = sum over windows of another class of exp(s[n, k]),  H[k] = sum over groups of 1 / (exp(pos[b, k]) + G[k])"""
    k = torch.arange(T, device=logits.device)
    neg = (labels[:T].reshape(T, 1) != k.reshape(1, T)).to(logits.dtype)
    Gk = (logits.exp() * neg).sum(dim=(0, 1))
    pos = logits[:, k, k]
    return torch.stack([Gk, (1.0 / (pos.exp() + Gk)).sum(0)])


def loss_of_logits(logits: torch.Tensor, labels: torch.Tensor, gneg: Union[None, bool, torch.Tensor] = None) -> torch.Tensor:
    G = logits.shape[0]
    y = labels[:T]
    tgt = y.repeat(G)
    row = F.cross_entropy(logits.reshape(-1, T), tgt)
    if gneg is None or gneg is False:
        col = F.cross_entropy(logits.transpose(1, 2).reshape(-1, T), tgt)
        return (row + col) / 2
    assert torch.equal(y.cpu(), torch.arange(T)), "global negatives are defined for the identity layout"
    k = torch.arange(T, device=logits.device)
    pos = logits[:, k, k]                                                         # (G, 41): the positive of column k
    if gneg is True:
        neg = (1.0 - torch.eye(T, dtype=logits.dtype, device=logits.device))
        Gk = (logits.exp() * neg).sum(dim=(0, 1))
        col = (-pos + torch.log(pos.exp() + Gk)).mean()
    else:
        Gk, Hk = gneg[0, :T].to(logits.dtype).detach(), gneg[1, :T].to(logits.dtype).detach()
        col = (-pos + torch.log(pos.exp() + Gk)).mean()
        # G is a constant here; what its dependence on every negative logit adds to the gradient, exp(s[n, k]) H[k] / (G 41), enters
        # through a term of value zero
        neg = (1.0 - torch.eye(T, dtype=logits.dtype, device=logits.device))
        through_g = (logits.exp() * neg * Hk).sum() / (G * T)
        col = col + through_g - through_g.detach()
    return (row + col) / 2


def loss_per_group(logits: torch.Tensor, labels: torch.Tensor, gneg: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(G,): every group's share of the loss; their mean is loss_of_logits (gneg: the {G, H} table, G taken as given)"""
    G = logits.shape[0]
    tgt = labels[:T].repeat(G)
    row = F.cross_entropy(logits.reshape(-1, T), tgt, reduction="none").reshape(G, T).mean(1)
    if gneg is None:
        col = F.cross_entropy(logits.transpose(1, 2).reshape(-1, T), tgt, reduction="none").reshape(G, T).mean(1)
    else:
        k = torch.arange(T, device=logits.device)
        pos = logits[:, k, k]
        col = (-pos + torch.log(pos.exp() + gneg[0, :T].to(logits.dtype))).mean(1)
    return (row + col) / 2


def _summary(logits: torch.Tensor, labels: torch.Tensor) -> Dict[str, torch.Tensor]:
    pred = logits.argmax(-1)                                                      # first maximum
    top2 = logits.topk(2, dim=-1).values
    return dict(pred=pred, correct=(pred == labels[:T][None]).sum(), margin=top2[..., 0] - top2[..., 1])


def head_reference(z, labels, V, easy_w=None, easy_b=None, zg=None, gneg=None, want_grad=True,
                   dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """-> logits (G,41,41), loss, correct, pred (G,41), margin (G,41: top-2 gap of every row), and with want_grad dz (n,16) and
    d_easy_w (16,41) / d_easy_b (16,), or dzg (B*41,16); with gneg also gh (2,41).  dtype=torch.float32 is the same formulas
    in single precision (the yardstick for a single-precision kernel's error)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(want_grad)
    z = leaf(z)
    if zg is not None:
        cls = [leaf(zg)]
        logits = head_logits(z, labels, V, zg=cls[0])
    else:
        cls = [leaf(easy_w), leaf(easy_b)]
        logits = head_logits(z, labels, V, cls[0], cls[1])
    loss = loss_of_logits(logits, labels, gneg)
    out = dict(logits=logits.detach(), loss=loss.detach(), **_summary(logits.detach(), labels))
    if gneg is not None and gneg is not False:
        out["gh"] = gneg_table(logits.detach(), labels) if gneg is True else gneg[:, :T].to(dtype)
    if want_grad:
        grads = torch.autograd.grad(loss, [z] + cls)
        out["dz"] = grads[0]
        if zg is not None:
            out["dzg"] = grads[1]
        else:
            out["d_easy_w"], out["d_easy_b"] = grads[1], grads[2]
    return out


def head_from_logits(logits, z, labels, V, easy_w=None, easy_b=None, zg=None, gneg=None,
                     dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The straight-through head: everything that is a function of the logits from `logits` as given, the gradients with
    dl = dL/dlogits pushed through the UNQUANTISED z_hat . e_hat."""
    given = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = loss_of_logits(given, labels, gneg)
    dl, = torch.autograd.grad(loss, given)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    z = leaf(z)
    if zg is not None:
        cls = [leaf(zg)]
        true = head_logits(z, labels, V, zg=cls[0])
    else:
        cls = [leaf(easy_w), leaf(easy_b)]
        true = head_logits(z, labels, V, cls[0], cls[1])
    grads = torch.autograd.grad((dl * true).sum(), [z] + cls)
    out = dict(logits=given.detach(), loss=loss.detach(), dl=dl, dz=grads[0], **_summary(given.detach(), labels))
    if zg is not None:
        out["dzg"] = grads[1]
    else:
        out["d_easy_w"], out["d_easy_b"] = grads[1], grads[2]
    return out
