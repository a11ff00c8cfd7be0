"""The adaptive multi-stream online decoder on the MI355X (contrastiveprosthetics_amd/online.py AdaptiveMultiStreamDecoder,
csrc/online_multi_adapt.cuh): after every push, every stream's pred, voted, logits, windows and BatchNorm statistics equal
bit for bit those of its own OnlineDecoder(adapt=alpha_s) with the same class table and calibration fed that stream alone;
stream isolation under calibrate / set_alpha / reset_statistics; reset, refresh and hand-over; refusals; launches per push."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 2400
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)


def _train_steps(e, steps, seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(41).repeat(4).cuda()
    for _ in range(steps):
        x = (torch.randn(4 * 41, 12, generator=g) * 1.5 + 0.3).cuda()
        z = e.encoder_forward(x, training=True)
        if e.class_encoder == "glove":
            zg = e.glove_forward((torch.randn(4, 41, 20, generator=g)).cuda(), training=True)
            e.head_glove(z, zg, labels, 1, want_grad=True)
            e.glove_backward()
        else:
            e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(PARAMS)


def _engine(adabn, seed=3, class_encoder="onehot", steps=3):
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=adabn, dtype="f32", device="cuda:0", seed=seed, class_encoder=class_encoder)
    e.init_parameters(seed)
    _train_steps(e, steps, seed)
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def stock():
    return _engine(False, seed=3, class_encoder="glove")       # one-hot, glove and raw tables


@pytest.fixture(scope="module")
def ada():
    return _engine(True, seed=5)


def _recordings(n, seed=11, length=L):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((rng.standard_normal((length, 12)) * (1 + 0.2 * i) * 2e-3).astype(np.float32)).cuda()
            for i in range(n)]


@pytest.fixture(scope="module")
def norm():
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rec = _recordings(1, seed=5)[0]
    w = preprocess_segments(rec[None], keep=20 * np.arange(110))[0]
    return w.mean(0), w.std(0)


def _schedule(n_streams, n_pushes, seed, idle=0.3, hi=400, length=L):
    """per push, the chunk size of every stream (0: idle), random per stream, until each recording is used up"""
    rng = np.random.default_rng(seed)
    left = np.full(n_streams, length)
    pushes = []
    for _ in range(n_pushes):
        n = rng.integers(1, hi, n_streams) * (rng.random(n_streams) >= idle)
        n = np.minimum(n, left)
        left -= n
        pushes.append(n)
    pushes.append(left.copy())
    return pushes


def _set(dec, s, spec, single=False):
    if "classes" in spec:
        args = dict(classes=spec["classes"])
    elif "glove" in spec:
        args = dict(glove=torch.randn(spec["glove"], 20, generator=torch.Generator().manual_seed(8 + s)))
    else:
        g = torch.Generator().manual_seed(100 + s)
        t = torch.randn(spec["k"], 16, generator=g)
        ids = None if spec["ids"] is None else (torch.randperm(64, generator=g)[:spec["k"]] + 3).tolist()
        args = dict(table=t, ids=ids)
    if single:
        dec.set_classes(**args)
    else:
        dec.set_classes(s, **args)


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape, (what, i, x.shape, y.shape)
        assert torch.equal(x, y), (what, i)


def _lockstep(dec, refs, recs, pushes, pos=None, check=None):
    """push `pushes` into dec and every reference decoder; after every push compare outputs and statistics of the streams
    in refs (a dict stream -> OnlineDecoder)"""
    pos = np.zeros(len(recs), dtype=np.int64) if pos is None else pos
    for t, n in enumerate(pushes):
        chunks = [None] * dec.n_streams
        for s in range(len(recs)):
            if n[s] or s % 2:                                  # idle streams as None and as empty tensors
                chunks[s] = recs[s][pos[s]:pos[s] + n[s]]
        out = dec.push(chunks, return_logits=True, return_windows=True)
        for s, ref in refs.items():
            if n[s]:
                r = ref.push(recs[s][pos[s]:pos[s] + n[s]], return_logits=True, return_windows=True)
                _same(out[s], r, (t, s))
            else:
                assert out[s][0].shape[0] == 0
            _same([dec.bn_statistics(s)], [ref.bn_statistics()], ("statistics", t, s))
        pos += n
    return pos


STOCK_TABLES = [dict(classes=list(range(41))), dict(glove=12), dict(table=True, k=12, ids="perm"), dict(classes=[30, 2, 17, 5, 9]),
                dict(glove=3), dict(table=True, k=64, ids=None)]
ADA_TABLES = [dict(classes=list(range(41))), dict(table=True, k=12, ids="perm"), dict(classes=[7]), dict(classes=[40, 0, 21]),
              dict(table=True, k=5, ids=None), dict(classes=list(range(0, 41, 3)))]
ALPHAS = [0.05, 0.0, 0.2, 0.01, 0.5, 0.001]


@pytest.mark.parametrize("model", ["stock", "adabn"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_streams_bit_identical_to_adaptive_decoders(stock, ada, norm, dtype, model):
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, OnlineDecoder
    mean, std = norm
    e = stock if model == "stock" else ada
    tables = STOCK_TABLES if model == "stock" else ADA_TABLES
    S = len(tables)
    recs = _recordings(S, seed=21)
    cals = _recordings(S, seed=22, length=1500)                # a different calibration recording per stream
    dec = AdaptiveMultiStreamDecoder(e, mean, std, S, ALPHAS, dtype=dtype)
    refs = {}
    for s, spec in enumerate(tables):
        _set(dec, s, spec)
        refs[s] = OnlineDecoder(e, mean, std, dtype=dtype, adapt=ALPHAS[s])
        _set(refs[s], s, spec, single=True)
        if model == "adabn" or s % 2:                          # the stock model: some streams calibrated, some not
            dec.calibrate(s, cals[s])
            refs[s].calibrate(cals[s])
    for s in range(S):
        _same([dec.bn_statistics(s)], [refs[s].bn_statistics()], ("initial", s))
    _lockstep(dec, refs, recs, _schedule(S, 10, seed=1 if dtype == "f32" else 2))
    assert list(dec.n_seen) == [L] * S


def _fc_batches(seen, counts, phase=0):
    """The most batches one workgroup of an fc launch runs for this push: the row blocks of olam_fc_blocks (about 16 of
    them) and the batches of at most 256 rows of olam_fc_kernel, restated on the host.  >= 2: the multi-batch branch runs."""
    from contrastiveprosthetics_amd.online import packed_rows
    row0, m = packed_rows(seen, counts, phase)
    R = int(m.sum())
    if R == 0:
        return 0
    b = min(16, R)
    rpb = (R + b - 1) // b
    most = 0
    for blk in range((R + rpb - 1) // rpb):
        mine = [s for s in range(len(m)) if m[s] > 0 and blk * rpb <= row0[s] < (blk + 1) * rpb]
        if not mine:
            continue
        last, s, n = mine[-1], mine[0], 0
        while s <= last:
            e = s + 1
            while e <= last and row0[e] + m[e] - row0[s] <= 256:
                e += 1
            n, s = n + 1, e
        most = max(most, n)
    return most


@pytest.mark.parametrize("dtype,model", [("bf16", "stock"), ("f32", "adabn")])
def test_256_streams_every_stream(stock, ada, norm, dtype, model):
    """all 256 streams against their own decoders: one-window ticks, a 25-window push of every stream (6,400 rows: each fc
    workgroup runs two batches) and random chunkings with idle streams"""
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, OnlineDecoder
    mean, std = norm
    e = stock if model == "stock" else ada
    S = 256
    pushes = [np.full(S, 20)] * 3 + [np.full(S, 500)]
    rng = np.random.default_rng(7)
    for _ in range(3):
        pushes.append(rng.integers(1, 120, S) * (rng.random(S) >= 0.3))
    length = int(np.sum(pushes, axis=0).max())
    recs = _recordings(S, seed=31, length=length)
    alphas = [0.0 if s % 5 == 0 else 0.001 * (1 + s % 7) for s in range(S)]
    table = lambda s: [s % 41, (s * 7 + 3) % 41, 40 - s % 41] if s % 41 != 20 else [20]     # noqa: E731
    dec = AdaptiveMultiStreamDecoder(e, mean, std, S, alphas, dtype=dtype, max_rows=S * 25)
    cals = _recordings(S, seed=34, length=600) if model == "adabn" else None
    refs = {}
    for s in range(S):
        dec.set_classes(s, classes=table(s))
        refs[s] = OnlineDecoder(e, mean, std, dtype=dtype, adapt=alphas[s])
        refs[s].set_classes(classes=table(s))
        if cals is not None or s % 64 == 3:
            cal = cals[s] if cals is not None else recs[(s + 1) % S]
            dec.calibrate(s, cal)
            refs[s].calibrate(cal)
    seen = np.zeros(S, dtype=np.int64)
    assert _fc_batches(seen + 60, pushes[3]) == 2
    _lockstep(dec, refs, recs, pushes)


@pytest.mark.parametrize("dtype,model", [("f32", "adabn"), ("bf16", "stock")])
def test_fc_row_blocks_over_256_rows(stock, ada, norm, dtype, model):
    """pushes of 40 streams of up to 250 windows each, idle streams in between: the streams whose rows start in one fc row
    block span more than 256 rows, so a workgroup runs them in several batches"""
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, OnlineDecoder
    mean, std = norm
    e = stock if model == "stock" else ada
    S, length = 40, 11000
    rng = np.random.default_rng(8 if dtype == "f32" else 9)
    pushes = [rng.integers(1500, 5000, S) * (rng.random(S) >= 0.25) for _ in range(2)]
    pushes.append(length - pushes[0] - pushes[1])
    recs = _recordings(S, seed=81, length=length)
    alphas = [(0.0, 0.02, 0.3, 0.001, 0.1)[s % 5] for s in range(S)]
    dec = AdaptiveMultiStreamDecoder(e, mean, std, S, alphas, dtype=dtype, max_rows=S * 256)
    tables = STOCK_TABLES if model == "stock" else ADA_TABLES
    cals = _recordings(S, seed=82, length=900)
    refs = {}
    for s in range(S):
        _set(dec, s, tables[s % len(tables)])
        refs[s] = OnlineDecoder(e, mean, std, dtype=dtype, adapt=alphas[s])
        _set(refs[s], s, tables[s % len(tables)], single=True)
        if model == "adabn" or s % 3 == 0:
            dec.calibrate(s, cals[s])
            refs[s].calibrate(cals[s])
    seen = np.zeros(S, dtype=np.int64)
    for n in pushes[:2]:
        assert _fc_batches(seen, n) >= 2
        seen += n
    _lockstep(dec, refs, recs, pushes)


def test_host_split(ada, norm):
    """a push above max_rows and above max_windows_per_push for one stream is split on the host (AdaBN, f32)"""
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, OnlineDecoder
    mean, std = norm
    S = 6
    recs = _recordings(S, seed=32)
    cals = _recordings(S, seed=33, length=1200)
    small = AdaptiveMultiStreamDecoder(ada, mean, std, S, ALPHAS, max_windows_per_push=16, max_rows=40)
    refs = {}
    for s, spec in enumerate(ADA_TABLES):
        _set(small, s, spec)
        small.calibrate(s, cals[s])
        refs[s] = OnlineDecoder(ada, mean, std, adapt=ALPHAS[s])
        _set(refs[s], s, spec, single=True)
        refs[s].calibrate(cals[s])
    _lockstep(small, refs, recs, _schedule(S, 4, seed=5, idle=0.2, hi=900))


def test_isolation_under_calibrate_alpha_and_reset_statistics(stock, norm):
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, OnlineDecoder
    mean, std = norm
    S, K = 5, 2
    recs = _recordings(S, seed=41)
    cal = _recordings(1, seed=42, length=1300)[0]
    alphas = [0.02, 0.1, 0.05, 0.0, 0.3]
    dec = AdaptiveMultiStreamDecoder(stock, mean, std, S, alphas)
    refs = {}
    for s in range(S):
        dec.set_classes(s, classes=list(range(41)))
        refs[s] = OnlineDecoder(stock, mean, std, classes=list(range(41)), adapt=alphas[s])
    pushes = _schedule(S, 8, seed=6)
    pos = _lockstep(dec, refs, recs, pushes[:4])
    others = {s: r for s, r in refs.items() if s != K}
    dec.calibrate(K, cal)                                      # stream K: calibrated mid-stream ...
    k_ref = OnlineDecoder(stock, mean, std, classes=list(range(41)), adapt=alphas[K])
    k_ref.calibrate(cal)
    assert torch.equal(dec.bn_statistics(K), k_ref.bn_statistics())
    pos = _lockstep(dec, others, recs, pushes[4:6], pos=pos)
    dec.set_alpha(K, 0.4)                                      # ... a new alpha ...
    pos = _lockstep(dec, others, recs, pushes[6:7], pos=pos)
    dec.reset_statistics(K)                                    # ... and handed over
    fresh = OnlineDecoder(stock, mean, std, classes=list(range(41)), adapt=0.4)
    assert torch.equal(dec.bn_statistics(K), fresh.bn_statistics())
    _lockstep(dec, others, recs, pushes[7:], pos=pos)


def test_reset_refresh_keep_statistics_and_handover(norm):
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, OnlineDecoder
    mean, std = norm
    for adabn in (False, True):
        e = _engine(adabn, seed=6)
        recs = _recordings(3, seed=51)
        dec = AdaptiveMultiStreamDecoder(e, mean, std, 3, [0.05, 0.0, 0.02])
        for s in range(3):
            dec.set_classes(s, classes=list(range(41)))
            if adabn:
                dec.calibrate(s, recs[(s + 1) % 3][:1500])
        a = dec.push([r[:1500] for r in recs], return_logits=True)
        st = [dec.bn_statistics(s) for s in range(3)]
        dec.reset()
        assert all(torch.equal(dec.bn_statistics(s), st[s]) for s in range(3))
        _train_steps(e, 1, 99)
        dec.refresh()
        assert all(torch.equal(dec.bn_statistics(s), st[s]) for s in range(3))
        dec.reset()
        b = dec.push([r[:1500] for r in recs], return_logits=True)
        assert not torch.equal(a[0][2], b[0][2])
        # a slot handed to a new user behaves as a freshly built OnlineDecoder(adapt=alpha) of the current model
        dec.reset_statistics(2)
        dec.reset(streams=[2])
        fresh = OnlineDecoder(e, mean, std, classes=list(range(41)), adapt=0.02)
        assert torch.equal(dec.bn_statistics(2), fresh.bn_statistics())
        if adabn:
            dec.calibrate(2, recs[0][:1500])
            fresh.calibrate(recs[0][:1500])
        for p in range(0, 1500, 500):
            o = dec.push([None, None, recs[2][p:p + 500]], return_logits=True, return_windows=True)[2]
            _same(o, fresh.push(recs[2][p:p + 500], return_logits=True, return_windows=True), ("fresh", adabn, p))
            assert torch.equal(dec.bn_statistics(2), fresh.bn_statistics())


def test_refusals_enqueue_nothing(ada, stock, norm):
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, MultiStreamDecoder, _lib
    mean, std = norm
    recs = _recordings(3, seed=61)
    with pytest.raises(_lib.CpNativeError, match="8-bit"):
        AdaptiveMultiStreamDecoder(ada, mean, std, 2, 0.01, dtype="fp8")
    for bad in (1.0, -0.1, [0.1, 1.0], [0.1]):
        with pytest.raises(ValueError):
            AdaptiveMultiStreamDecoder(stock, mean, std, 2, bad)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="n_streams"):
            AdaptiveMultiStreamDecoder(stock, mean, std, bad, 0.01)
    with pytest.raises(_lib.CpNativeError, match="AdaBN"):
        MultiStreamDecoder(ada, mean, std, 2)                   # the folded form keeps its refusals
    with pytest.raises(_lib.CpNativeError, match="adapt"):
        MultiStreamDecoder(stock, mean, std, 2, adapt=0.01)
    d = AdaptiveMultiStreamDecoder(ada, mean, std, 3, [0.01, 0.02, 0.0])
    ref = AdaptiveMultiStreamDecoder(ada, mean, std, 3, [0.01, 0.02, 0.0])
    for x in (d, ref):
        x.set_classes(0, classes=list(range(41)))
        x.set_classes(2, classes=[1, 2, 3])
        x.calibrate(2, recs[1][:1500])
    torch.cuda.synchronize()
    ws0 = d.ws.clone()
    with pytest.raises(_lib.CpNativeError, match="calibrate"):
        d.push([recs[0][:100], None, recs[2][:100]])            # stream 0 is uncalibrated
    with pytest.raises(_lib.CpNativeError, match="AdaBN"):
        d.set_classes(1, glove=torch.randn(3, 20))
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            d.set_alpha(1, bad)
    with pytest.raises(ValueError, match="at least 2 windows"):
        d.calibrate(0, recs[0][:30])
    for bad in (3, -1, 1.0):
        with pytest.raises(IndexError):
            d.calibrate(bad, recs[0][:1500])
        with pytest.raises(IndexError):
            d.bn_statistics(bad)
        with pytest.raises(IndexError):
            d.reset_statistics(bad)
    with pytest.raises(_lib.CpNativeError, match="no class table"):
        d.push([None, recs[1][:100], None])
    torch.cuda.synchronize()
    assert torch.equal(d.ws, ws0)                               # nothing was enqueued
    assert list(d.n_seen) == [0, 0, 0]
    chunks = [None, None, recs[2][:700]]                        # an idle uncalibrated stream is fine
    o, r = d.push(chunks, return_logits=True), ref.push(chunks, return_logits=True)
    _same(o[2], r[2], "after refusals")
    assert torch.equal(d.bn_statistics(2), ref.bn_statistics(2))


def test_launches_per_push_do_not_depend_on_streams(stock, norm):
    from torch.profiler import ProfilerActivity, profile
    from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder
    mean, std = norm
    counts = {}
    for S in (1, 8, 64):
        recs = _recordings(1, seed=71, length=20 * 4 * S)[0]
        dec = AdaptiveMultiStreamDecoder(stock, mean, std, S, 0.01, max_rows=S)
        for s in range(S):
            dec.set_classes(s, classes=list(range(41)))
        push = lambda p: dec.push_packed(recs[p * 20 * S:(p + 1) * 20 * S], [20] * S)    # noqa: E731
        push(0)                                                 # the device copy of the counts is made once
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for p in range(1, 4):
                push(p)
            torch.cuda.synchronize()
        names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
                 and "Memcpy" not in ev.name and "Memset" not in ev.name]
        counts[S] = len(names) / 3
        print(S, counts[S], sorted(set(names)))
    assert counts[1] == counts[8] == counts[64], counts
    assert counts[1] <= 12, counts
