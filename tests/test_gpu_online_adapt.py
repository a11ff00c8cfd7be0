"""The adaptive online decoder on the MI355X (OnlineDecoder(..., adapt=alpha), csrc/online_adapt.cuh): an AdaBN model decodes
live after calibration and matches the reference's AdaBN eval on the same batch, calibration statistics against a float64
forward, the frozen adaptive form against the folded one, tracking against a float64 restatement of the recurrence, chunk
invariance, and what reset / refresh / refusals do."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

L = 5130
N_CAL = 246                                  # windows of the calibration recording: 6 groups of 41
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
EPS = 1e-5


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
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rng = np.random.default_rng(11)
    rec = torch.from_numpy((rng.standard_normal((L, 12)) * 2e-3).astype(np.float32)).cuda()
    w = preprocess_segments(rec[None], keep=20 * np.arange(256))[0]
    return rec, w.mean(0), w.std(0)


def _table(e):
    return e.values.views["glove_net.easy.0.weight"].t() + e.values.views["glove_net.easy.0.bias"]


def _ref_logits(engine, windows, table):
    n = windows.shape[0]
    assert n % 41 == 0                                            # the encoder takes whole groups of 41 rows
    z = engine.encoder_forward(windows.contiguous(), training=False)[:n]
    zn = z / z.norm(dim=-1, keepdim=True)
    tn = table / table.norm(dim=-1, keepdim=True)
    return zn @ tn.t()


def _cal_samples(n_windows):
    from contrastiveprosthetics_amd.online import windows_before
    n = 20 * n_windows
    while windows_before(n) > n_windows:
        n -= 1
    assert windows_before(n) == n_windows
    return n


def test_adabn_model_decodes_live(ada, recording):
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    cal = rec[:_cal_samples(N_CAL)]
    dec = OnlineDecoder(ada, mean, std, classes=list(range(41)), dtype="f32", adapt=0.0)
    dec.calibrate(cal)
    dec.reset()
    pred, voted, logits, win = dec.push(cal, return_logits=True, return_windows=True)
    assert win.shape[0] == N_CAL
    assert torch.equal(win, dec.calibration_windows(cal))
    ref = _ref_logits(ada, win, _table(ada))                       # the reference's AdaBN eval on the same batch
    dev = float((logits - ref).abs().max())
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    print(f"AdaBN: adaptive decoder (calibrated, alpha 0) vs encoder_forward(eval): max |logit diff| {dev:.3e}, "
          f"{int(clear.sum())} of {N_CAL} windows clear")
    assert dev <= 1e-4
    assert torch.equal(pred[clear].long(), ref.argmax(1)[clear])


def _f64_batch_statistics(e, windows):
    """float64 CPU forward of the AdaBN model on one batch: each layer's batch mean and biased variance in turn"""
    from oracle.ref_cpu import OracleModel
    sd = {k: v.detach().double().cpu() for k, v in e.values.views.items()}
    om = OracleModel(sd, PARAMS, adabn=True)
    om.set_test()
    taps = {}
    with torch.no_grad():
        om.encode_emg(windows.double().cpu().reshape(1, 1, -1, 12), taps)
    out = torch.zeros(9, 2, 512, dtype=torch.float64)
    for l in range(9):
        r = taps[f"r{l}"]
        dims = (0, 2, 3) if l < 2 else (0,)
        c = r.shape[1]
        out[l, 0, :c] = r.mean(dims)
        out[l, 1, :c] = r.var(dims, unbiased=False)
    return out


def test_calibration_statistics(ada, recording):
    """over more than one chunk of 256 windows, so the float64 merges across chunks are checked too"""
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    cal = torch.cat([rec, rec[:1500] * 0.6 + 1e-4]).contiguous()
    dec = OnlineDecoder(ada, mean, std, classes=list(range(41)), dtype="f32", adapt=0.0)
    dec.calibrate(cal)
    got = dec.bn_statistics().cpu()
    ref = _f64_batch_statistics(ada, dec.calibration_windows(cal))
    mu, v, rmu, rv = got[:, 0], got[:, 1], ref[:, 0], ref[:, 1]
    dmu = ((mu - rmu).abs() / rv.sqrt().clamp_min(1e-30)).max(dim=1).values
    dv = ((v - rv).abs() / rv.clamp_min(1e-30)).max(dim=1).values
    print("calibration vs float64 forward, per BN: max |dmu|/sqrt(v)", [f"{x:.1e}" for x in dmu.tolist()],
          "max |dv|/v", [f"{x:.1e}" for x in dv.tolist()])
    live = rv > 0
    assert bool(((mu - rmu).abs() <= 1e-5 * rv.sqrt())[live].all())
    assert bool(((v - rv).abs() <= 1e-5 * rv)[live].all())
    assert bool((mu[~live] == rmu[~live]).all()) and bool((v[~live] == 0).all())      # dead channels and unused slots


def test_frozen_adaptive_equals_folded(stock, recording):
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    fold = OnlineDecoder(stock, mean, std, classes=list(range(41)), dtype="f32")
    ad = OnlineDecoder(stock, mean, std, classes=list(range(41)), dtype="f32", adapt=0.0)
    st = ad.bn_statistics()
    for l, base in enumerate(_bn_bases()):
        c = 64 if l < 2 else 512
        assert torch.equal(st[l, 0, :c], stock.running[base + ".running_mean"].double())
        assert torch.equal(st[l, 1, :c], stock.running[base + ".running_var"].double())
    pf, _, lf = fold.push(rec, return_logits=True)
    pa, _, la = ad.push(rec, return_logits=True)
    dev = float((la - lf).abs().max())
    top2 = lf.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    print(f"adaptive (alpha 0) vs folded, f32: max |logit diff| {dev:.3e}")
    assert dev <= 1e-4
    assert torch.equal(pa[clear], pf[clear])
    assert torch.equal(ad.bn_statistics(), st)                       # alpha 0 freezes them
    a16 = OnlineDecoder(stock, mean, std, classes=list(range(41)), dtype="bf16", adapt=0.0)
    p16, _, l16 = a16.push(rec, return_logits=True)
    dev16, agree = float((l16 - la).abs().max()), float((p16 == pa).float().mean())
    print(f"adaptive bf16 vs f32: max |logit diff| {dev16:.3e}, argmax agreement {agree:.4f}")
    assert dev16 <= 2e-2
    assert agree >= 0.99


def _bn_bases():
    from contrastiveprosthetics_amd.engine import bn_bases
    return bn_bases(False)


def _f64_tracking(e, windows, table, alpha):
    """The push recurrence of include/cpnative.h restated in float64: per window, per BN in layer order, normalise with the
    statistics before the window, then mu += alpha d, v = (1 - alpha)(v + alpha d^2) + alpha w."""
    P = {k: v.detach().double().cpu() for k, v in e.values.views.items()}
    bases = _bn_bases()
    mu = [e.running[b + ".running_mean"].double().cpu().clone() for b in bases]
    var = [e.running[b + ".running_var"].double().cpu().clone() for b in bases]
    fc = [(P[f"emg_net.linear.{i}.weight"], P[f"emg_net.linear.{i}.bias"]) for i in (0, 3, 6, 9, 13, 17, 21)]
    tn = table.double().cpu()
    tn = tn / tn.norm(dim=-1, keepdim=True)

    def bn(l, u):                                  # u: (C, P)
        g, b = P[bases[l] + ".weight"], P[bases[l] + ".bias"]
        y = g[:, None] * (u - mu[l][:, None]) / torch.sqrt(var[l][:, None] + EPS) + b[:, None]
        m, w = u.mean(1), u.var(1, unbiased=False)
        d = m - mu[l]
        mu[l] = mu[l] + alpha * d
        var[l] = (1 - alpha) * (var[l] + alpha * d * d) + alpha * w
        return y

    logits = []
    for x in windows.double().cpu():
        h = F.relu(F.conv2d(x.reshape(1, 1, 1, 12), P["emg_net.conv_emg.0.weight"], P["emg_net.conv_emg.0.bias"], padding=1))
        h = bn(0, h.reshape(64, 12)).reshape(1, 64, 1, 12)
        h = F.relu(F.conv2d(h, P["emg_net.conv_emg.3.weight"], P["emg_net.conv_emg.3.bias"], padding=1))
        h = bn(1, h.reshape(64, 12)).reshape(-1)
        for i, (W, b) in enumerate(fc):
            h = bn(2 + i, F.relu(W @ h + b)[:, None])[:, 0]
        z = P["emg_net.last.0.weight"] @ h
        logits.append((z / z.norm()) @ tn.t())
    stats = torch.zeros(9, 2, 512, dtype=torch.float64)
    for l in range(9):
        stats[l, 0, :mu[l].numel()], stats[l, 1, :var[l].numel()] = mu[l], var[l]
    return torch.stack(logits), stats


@pytest.fixture(scope="module")
def drifting(recording):
    """the recording with channel gains and offsets that change halfway"""
    rec = recording[0].clone()
    g = torch.Generator().manual_seed(4)
    gain = (torch.rand(12, generator=g) * 1.5 + 0.5).cuda()
    off = (torch.randn(12, generator=g) * 1e-3).cuda()
    rec[L // 2:] = rec[L // 2:] * gain + off
    return rec


def test_tracking_against_f64_oracle(stock, recording, drifting):
    from contrastiveprosthetics_amd import OnlineDecoder
    _, mean, std = recording
    alpha = 0.01
    dec = OnlineDecoder(stock, mean, std, classes=list(range(41)), dtype="f32", adapt=alpha)
    pred, _, logits, win = dec.push(drifting, return_logits=True, return_windows=True)
    ref, ref_stats = _f64_tracking(stock, win, _table(stock), alpha)
    got_stats = dec.bn_statistics().cpu()
    dev = float((logits.double().cpu() - ref).abs().max())
    mu, v, rmu, rv = got_stats[:, 0], got_stats[:, 1], ref_stats[:, 0], ref_stats[:, 1]
    dmu = float(((mu - rmu).abs() / (rmu.abs() + rv.sqrt()).clamp_min(1e-30)).max())
    dv = float(((v - rv).abs() / rv.clamp_min(1e-30)).max())
    print(f"tracking, alpha {alpha}: max |logit diff| vs float64 {dev:.3e} over {win.shape[0]} windows; "
          f"final statistics: max |dmu|/(|mu|+sqrt(v)) {dmu:.2e}, max |dv|/v {dv:.2e}")
    assert dev <= 1e-4
    assert dmu <= 1e-6 and dv <= 1e-6
    frozen = OnlineDecoder(stock, mean, std, classes=list(range(41)), dtype="f32", adapt=0.0)
    _, _, l0 = frozen.push(drifting, return_logits=True)
    moved = float((l0 - logits).abs().max())
    print(f"alpha {alpha} vs alpha 0: max |logit diff| {moved:.3e}")
    assert moved > 1e-2                                              # adaptation is live


def _chunks(name, seed=0):
    if name == "whole":
        return [L]
    if name == "random":
        rng = np.random.default_rng(seed)
        out, s = [], 0
        while s < L:
            n = int(min(rng.integers(1, 400), L - s))
            out.append(n)
            s += n
        return out
    n = int(name)
    return [n] * (L // n) + ([L % n] if L % n else [])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_chunk_invariance(stock, recording, drifting, dtype):
    from contrastiveprosthetics_amd import OnlineDecoder
    _, mean, std = recording
    base = None
    for name in ("whole", "1", "7", "333", "random"):
        dec = OnlineDecoder(stock, mean, std, classes=list(range(41)), dtype=dtype, adapt=0.02)
        outs, s = [], 0
        for n in _chunks(name):
            outs.append(dec.push(drifting[s:s + n], return_logits=True))
            s += n
        res = [torch.cat([o[i] for o in outs]) for i in range(3)] + [dec.bn_statistics()]
        if base is None:
            base = res
            assert res[0].shape[0] == (L + 9) // 20
        else:
            for a, b, what in zip(res, base, ("pred", "voted", "logits", "statistics")):
                assert torch.equal(a, b), (name, what)


def test_reset_and_refresh_keep_statistics(recording):
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    e = _engine(False, seed=6)
    dec = OnlineDecoder(e, mean, std, classes=list(range(41)), adapt=0.05)
    a = dec.push(rec[:1500], return_logits=True)
    s1 = dec.bn_statistics()
    dec.reset()
    assert torch.equal(dec.bn_statistics(), s1)
    _train_steps(e, 1, 99)
    dec.refresh()
    assert torch.equal(dec.bn_statistics(), s1)
    dec.reset()
    b = dec.push(rec[:1500], return_logits=True)
    assert not torch.equal(a[2], b[2])


def test_refusals_on_the_device(ada, stock, recording):
    from contrastiveprosthetics_amd import OnlineDecoder, _lib
    rec, mean, std = recording
    with pytest.raises(_lib.CpNativeError, match="AdaBN"):
        OnlineDecoder(ada, mean, std, classes=[1, 2])                    # the folded form still refuses AdaBN
    dec = OnlineDecoder(ada, mean, std, classes=list(range(41)), adapt=0.01)
    ws0 = dec.ws.clone()
    with pytest.raises(_lib.CpNativeError, match="calibrate"):
        dec.push(rec[:200])
    with pytest.raises(_lib.CpNativeError, match="AdaBN"):
        dec.set_classes(glove=torch.randn(3, 20))
    with pytest.raises(ValueError, match="at least 2 windows"):
        dec.calibrate(rec[:30])
    with pytest.raises(_lib.CpNativeError, match="8-bit"):
        OnlineDecoder(ada, mean, std, classes=[1, 2], dtype="fp8", adapt=0.01)
    with pytest.raises(ValueError):
        OnlineDecoder(stock, mean, std, classes=[1, 2], adapt=1.0)
    torch.cuda.synchronize()
    assert torch.equal(dec.ws, ws0)                                      # nothing was enqueued
    from contrastiveprosthetics_amd.online import windows_before
    dec.calibrate(rec[:2000])
    pred, voted = dec.push(rec[:200])
    assert pred.numel() == windows_before(200)
    with pytest.raises(_lib.CpNativeError, match="adaptive form"):
        OnlineDecoder(stock, mean, std, classes=[1, 2]).bn_statistics()


def test_calibration_windows_are_the_stream_windows(stock, recording):
    """calibrate() turns a recording of more than 256 windows into the windows a fresh stream emits"""
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    rec2 = torch.cat([rec, rec * 0.5]).contiguous()
    dec = OnlineDecoder(stock, mean, std, classes=list(range(41)), adapt=0.0)
    _, _, win = dec.push(rec2, return_windows=True)
    assert win.shape[0] > 256
    assert torch.equal(dec.calibration_windows(rec2), win)
