"""cp_config.record (include/cpnative.h, cp_forward_record): what a forward pass leaves for the backward pass over its workspace is
a host record the caller keeps beside the buffer, so any number of engines can interleave their forward and backward passes, and a
backward with no forward behind its record is refused before it launches anything."""
import ctypes as C

import pytest
import torch

from contrastiveprosthetics_amd import _lib

pytestmark = pytest.mark.gpu
T = 41


def _engine(i, groups=2):
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=True, dtype="bf16", dp_emg=0.0635, device="cuda", seed=100 + i)
    e.init_parameters(i)
    g = torch.Generator().manual_seed(1000 + i)
    x = torch.randn(groups * T, 12, generator=g).cuda()
    return e, x, torch.arange(T).repeat(groups).cuda()


def _forward(e, x, labels):
    e.step_count = 0                                   # the same dropout draw in every run of an engine
    z = e.encoder_forward(x, training=True)
    e.head(z, labels, 1, want_grad=True)
    e.grads.flat.fill_(float("nan"))


def test_many_engines_interleaved_match_each_engine_alone():
    """65 engines (more than any fixed table of workspaces would hold): every forward first, then every backward.  Each call succeeds
    and each engine's gradients equal, bit for bit, those of the same engine run alone."""
    engines = [_engine(i) for i in range(65)]
    alone = []
    for e, x, labels in engines:
        _forward(e, x, labels)
        e.encoder_backward(x)
        alone.append(e.grads.flat.clone())
    for e, x, labels in engines:
        _forward(e, x, labels)
    for e, x, labels in engines:
        e.encoder_backward(x)
    torch.cuda.synchronize()
    for i, (e, _, _) in enumerate(engines):
        emg = [k for k in e.specs if k.startswith("emg_net.")]
        got = torch.cat([e.grads.views[k].reshape(-1) for k in emg])
        want = torch.cat([alone[i][o:o + m] for k, (o, m) in e.grads.offsets.items() if k.startswith("emg_net.")])
        assert torch.isfinite(want).all(), i
        assert torch.equal(got, want), i


def test_backward_without_a_filled_record_is_refused():
    """A record no forward has filled -- a fresh engine's, the one that comes with a grown workspace -- and a NULL record are
    CP_ERR_ARG."""
    e, x, labels = _engine(0)
    with pytest.raises(_lib.CpNativeError, match="no cp_encoder_forward"):
        e.encoder_backward(x)
    _forward(e, x, labels)
    e.workspace(4 * x.shape[0])                        # a new buffer and a new, empty record: the forward's tensors are not in it
    with pytest.raises(_lib.CpNativeError, match="no cp_encoder_forward"):
        e.encoder_backward(x)
    cfg = e._cfg(x.shape[0], True)
    ws, nb = e._ws_args(cfg)
    cfg.record = None
    code = e.lib.cp_encoder_backward(C.byref(cfg), C.byref(e._p), x.data_ptr(), ws, nb, C.byref(e._g), e._stream())
    assert code == 10001 and b"record is NULL" in e.lib.cp_last_error()           # CP_ERR_ARG
