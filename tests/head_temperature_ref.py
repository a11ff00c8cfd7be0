"""The contrastive head with a temperature, in torch (float64 by default): autograd over exp(clamp(s)) * oracle.head_cpu.head_logits
fed to oracle.head_cpu.loss_of_logits.  Shared by tests/test_head_temperature_host.py (which anchors it) and
tests/test_gpu_head_temperature.py (which holds the kernels to it).

    s = logit_scale, S = ln 100, tau = exp(min(max(s, -S), S)),  logits = tau * cosines
    dL/ds = sum dl * logits inside [-S, S] (autograd through the clamp), 0 outside

`s` is a Python float: the float32 value the kernel reads, taken exactly.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import head_cpu as hc  # noqa: E402

T = 41
S_MAX = math.log(100.0)
# float32(ln 100) lies above ln 100; the largest float32 INSIDE [-S, S] is what "s = ln 100" means to a kernel that reads a float
_S32 = np.float32(S_MAX)
S_MAX_F32 = float(_S32 if float(_S32) <= S_MAX else np.nextafter(_S32, np.float32(0.0)))
SCALES = {"ln 0.5": float(np.float32(math.log(0.5))), "ln 1/0.07": float(np.float32(math.log(1.0 / 0.07))),
          "ln 100": S_MAX_F32, "5.0": 5.0}


def tau_of(s: float) -> float:
    return math.exp(min(max(float(s), -S_MAX), S_MAX))


def _finish(out, loss, logits, leaves, s_t, glove, want_grad):
    if not want_grad:
        return out
    grads = torch.autograd.grad(loss, leaves + [s_t, logits])
    out["dz"] = grads[0]
    if glove:
        out["dzg"] = grads[1]
    else:
        out["d_easy_w"], out["d_easy_b"] = grads[1], grads[2]
    dl = grads[-1]
    out["ds"] = grads[-2]
    out["dl_l"] = (dl * logits.detach()).sum(dim=(1, 2))          # (G,): every group's share of sum dl * logits
    out["abs_dl_l"] = (dl * logits.detach()).abs().sum()
    return out


def temp_reference(z, labels, V, s, easy_w=None, easy_b=None, zg=None, want_grad=True, dtype=torch.float64):
    """-> logits (scaled), cosines, loss, pred, correct, margin (of the COSINES), and with want_grad dz, d_easy_w / d_easy_b or
    dzg, ds (dL/ds through the clamp), dl_l (G,), abs_dl_l"""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(want_grad)
    zl = leaf(z)
    s_t = torch.tensor(float(s), dtype=dtype, device=z.device, requires_grad=want_grad)
    if zg is not None:
        cls = [leaf(zg)]
        cos = hc.head_logits(zl, labels, V, zg=cls[0])
    else:
        cls = [leaf(easy_w), leaf(easy_b)]
        cos = hc.head_logits(zl, labels, V, cls[0], cls[1])
    logits = torch.exp(torch.clamp(s_t, -S_MAX, S_MAX)) * cos
    loss = hc.loss_of_logits(logits, labels)
    top2 = cos.detach().topk(2, dim=-1).values
    pred = logits.detach().argmax(-1)
    out = dict(logits=logits.detach(), cosines=cos.detach(), loss=loss.detach(), pred=pred,
               correct=(pred == labels[:T][None]).sum(), margin=top2[..., 0] - top2[..., 1])
    return _finish(out, loss, logits, [zl] + cls, s_t, zg is not None, want_grad)


def temp_from_logits(logits, z, labels, V, s, easy_w, easy_b, dtype=torch.float64):
    """The straight-through head of the 8-bit logits with a temperature: loss, predictions and dl from `logits` as given (the
    kernel's quantised, scaled ones); dz and the table gradients push dl through tau * (unquantised cosines); dL/ds = sum dl *
    given logits inside [-S, S]."""
    given = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = hc.loss_of_logits(given, labels)
    dl, = torch.autograd.grad(loss, given)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    zl, cls = leaf(z), [leaf(easy_w), leaf(easy_b)]
    cos = hc.head_logits(zl, labels, V, cls[0], cls[1])
    grads = torch.autograd.grad((dl * (tau_of(s) * cos)).sum(), [zl] + cls)
    inside = -S_MAX <= float(s) <= S_MAX
    dl_l = (dl * given.detach()).sum(dim=(1, 2))
    pred = given.detach().argmax(-1)
    return dict(logits=given.detach(), loss=loss.detach(), pred=pred, correct=(pred == labels[:T][None]).sum(),
                dz=grads[0], d_easy_w=grads[1], d_easy_b=grads[2], dl_l=dl_l,
                ds=dl_l.sum() if inside else torch.zeros((), dtype=dtype, device=z.device),
                abs_dl_l=(dl * given.detach()).abs().sum())
