"""What sits on the offline transform, on a recording longer than 65,536 samples (33 s at 2 kHz: a usual calibration
recording): `_calibration_windows` (13 calls of cp_preprocess_emg with kept positions up to 66,080), the one-pass
`recording_windows` and a push give the same windows, equal to the numpy oracle's; `calibrate()` of the adaptive decoders
takes its statistics from those windows."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import preprocess_cpu as pp

pytestmark = pytest.mark.gpu

L = 66100                                    # windows 0..3,304 at phase 0; window 3,277 is the first past raw sample 65,536
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)


def _train_steps(e, steps, seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(41).repeat(4).cuda()
    for _ in range(steps):
        x = (torch.randn(4 * 41, 12, generator=g) * 1.5 + 0.3).cuda()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(PARAMS)


def _engine(adabn, seed=3, steps=3):
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=adabn, dtype="f32", device="cuda:0", seed=seed)
    e.init_parameters(seed)
    _train_steps(e, steps, seed)
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def stock():
    return _engine(False)


@pytest.fixture(scope="module")
def ada():
    return _engine(True, seed=5)


@pytest.fixture(scope="module")
def recording():
    """(raw (L, 12) on the GPU, raw on the host, mean, std): the normalisation from the first 256 windows"""
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rng = np.random.default_rng(17)
    host = (rng.standard_normal((L, 12)) * 2e-3).astype(np.float32)
    rec = torch.from_numpy(host).cuda()
    w = preprocess_segments(rec[None], keep=20 * np.arange(256))[0]
    return rec, host, w.mean(0), w.std(0)


@pytest.fixture(scope="module")
def fresh():
    """2,000 samples that are not part of the recording"""
    rng = np.random.default_rng(18)
    return torch.from_numpy((rng.standard_normal((2000, 12)) * 2e-3).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def oracle_series(recording):
    """the RMS series of the whole recording by the numpy oracle, (L - 10, 12) float32, before normalisation"""
    host = recording[1]
    b, a = pp.butter_bandpass()
    y = pp.lfilter_df2t(b, a, host * np.float32(pp.GAIN)).astype(np.float32)
    out = np.sqrt(pp.uniform_filter1d_nearest(np.square(y), pp.RMS_WINDOW))[pp.WINDOW_EDGE:-pp.WINDOW_EDGE]
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("phase", [0, 13])
def test_offline_windows_equal_one_pass_and_push_on_a_long_recording(stock, recording, oracle_series, phase):
    """The identity that lets calibrate() move to the one-pass windows.  Against the oracle the rows are compared bit for
    bit: mean and std are the same float32 numbers on both sides, and (x - mean) / std is one correctly rounded float32
    subtraction and one correctly rounded float32 division on the device (no contraction) as in numpy."""
    from contrastiveprosthetics_amd import OnlineDecoder
    from contrastiveprosthetics_amd.online import _calibration_windows, recording_windows, windows_before
    rec, _, mean, std = recording
    dec = OnlineDecoder(stock, mean, std, classes=list(range(41)), dtype="f32", phase=phase)
    K = windows_before(L, phase)
    assert K == len(range(phase, L - 10, 20)) and 20 * (K - 1) + phase > 65536
    w_off = _calibration_windows(rec, dec._b, dec._a, phase, dec.mean_std)
    w_one = recording_windows(rec, dec.mean_std, dec._b, dec._a, phase)
    w_push = dec.push(rec, return_windows=True)[2]
    assert tuple(w_off.shape) == tuple(w_one.shape) == tuple(w_push.shape) == (K, 12)
    assert torch.equal(w_one, w_push)
    rows = (w_off != w_one).any(dim=1).nonzero().reshape(-1)
    print(f"phase {phase}: {K} windows, offline vs one-pass: {rows.numel()} rows differ"
          + (f", the first at window {int(rows[0])} (raw sample {phase + 20 * int(rows[0])})" if rows.numel() else ""))
    assert torch.equal(w_off, w_one)
    m, s = mean.cpu().numpy(), std.cpu().numpy()
    assert m.dtype == np.float32 and s.dtype == np.float32
    ref = ((oracle_series[phase + 20 * np.arange(K)] - m) / s).astype(np.float32)
    first = 3277                                       # the first window past raw sample 65,536 (both phases)
    assert phase + 20 * first > 65536 > phase + 20 * (first - 1)
    for name, w in (("offline", w_off), ("one-pass", w_one)):
        got = w.cpu().numpy()
        bad = np.flatnonzero((got != ref).any(axis=1))
        print(f"phase {phase}: {name} windows vs the oracle: {bad.size} of {K} rows differ, max |diff| {np.abs(got - ref).max():.3e}")
        assert np.array_equal(got[first:], ref[first:]), name
        assert np.array_equal(got, ref), name


def _calibrate_with(dec, windows):
    """cp_online_adapt_calibrate on given windows: what OnlineDecoder.calibrate does after it has made its own"""
    from contrastiveprosthetics_amd import _lib
    w = windows.contiguous()
    scratch = torch.empty(dec.lib.cp_online_adapt_calibrate_scratch_bytes(w.shape[0], dec._cfg.dtype), dtype=torch.uint8,
                          device=dec.device)
    _lib.check(dec.lib.cp_online_adapt_calibrate(C.byref(dec._cfg), *dec._ws(), w.data_ptr(), w.shape[0], scratch.data_ptr(),
                                                 scratch.numel(), dec._stream()), "cp_online_adapt_calibrate")
    dec.calibrated = True


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_calibrate_on_a_long_recording(ada, recording, fresh, dtype):
    """calibrate() of a 33 s recording against the same calibration from the one-pass windows: calibration adds in a fixed
    order, so equal windows give equal statistics, bit for bit"""
    from contrastiveprosthetics_amd import OnlineDecoder
    from contrastiveprosthetics_amd.online import recording_windows
    rec, _, mean, std = recording
    A = OnlineDecoder(ada, mean, std, classes=list(range(41)), dtype=dtype, adapt=0.0)
    B = OnlineDecoder(ada, mean, std, classes=list(range(41)), dtype=dtype, adapt=0.0)
    A.calibrate(rec)
    _calibrate_with(B, recording_windows(rec, B.mean_std, B._b, B._a, B.phase))
    sa, sb = A.bn_statistics(), B.bn_statistics()
    assert bool(torch.isfinite(sa).all())
    assert bool((sb[:, 1] > 0).any())                                  # B was calibrated: the statistics are not the zeros of a new workspace
    print(f"{dtype}: calibrate() vs calibration from the one-pass windows: {int((sa != sb).sum())} of {sa.numel()} statistics differ")
    assert torch.equal(sa, sb)
    pa, va, la = A.push(fresh, return_logits=True)
    pb, vb, lb = B.push(fresh, return_logits=True)
    assert la.shape[0] == 100
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(va, vb)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_multi_stream_calibrate_on_a_long_recording(ada, recording, fresh, dtype):
    """AdaptiveMultiStreamDecoder.calibrate(s, raw) with the long recording on one stream of three, against that stream's
    own OnlineDecoder(adapt=alpha) and against the one-pass windows"""
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, OnlineDecoder
    from contrastiveprosthetics_amd.online import recording_windows
    rec, _, mean, std = recording
    alphas = [0.05, 0.01, 0.0]
    tables = [list(range(41)), [30, 2, 17, 5, 9], list(range(0, 41, 3))]
    cals = [rec[:1500], rec, rec[40000:42000] * 0.5]                   # the long recording on the middle stream
    dec = AdaptiveMultiStreamDecoder(ada, mean, std, 3, alphas, dtype=dtype)
    refs = []
    for s in range(3):
        dec.set_classes(s, classes=tables[s])
        dec.calibrate(s, cals[s])
        refs.append(OnlineDecoder(ada, mean, std, classes=tables[s], dtype=dtype, adapt=alphas[s]))
        refs[s].calibrate(cals[s])
    one = OnlineDecoder(ada, mean, std, classes=tables[1], dtype=dtype, adapt=alphas[1])
    _calibrate_with(one, recording_windows(rec, one.mean_std, one._b, one._a, one.phase))
    for s in range(3):
        assert torch.equal(dec.bn_statistics(s), refs[s].bn_statistics()), s
    assert torch.equal(dec.bn_statistics(1), one.bn_statistics())
    chunks = [fresh[:700], fresh, fresh[300:1500]]
    out = dec.push(chunks, return_logits=True, return_windows=True)
    for s in range(3):
        r = refs[s].push(chunks[s], return_logits=True, return_windows=True)
        assert len(out[s]) == len(r) == 4
        for i, (x, y) in enumerate(zip(out[s], r)):
            assert x.shape == y.shape and torch.equal(x, y), (s, i)
        assert torch.equal(dec.bn_statistics(s), refs[s].bn_statistics()), s
    assert torch.equal(out[1][2], one.push(fresh, return_logits=True)[2])
