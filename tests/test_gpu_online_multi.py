"""The multi-stream online decoder on the MI355X (contrastiveprosthetics_amd/online.py MultiStreamDecoder,
csrc/online_multi.cuh): every stream's pred, voted, logits and windows equal bit for bit those of a single-stream
OnlineDecoder fed that stream alone, whatever the other streams push and however the push is split; stream isolation;
refresh(); refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 3000
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


def _engine(seed=3, class_encoder="onehot", steps=3):
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=False, dtype="f32", device="cuda:0", seed=seed, class_encoder=class_encoder)
    e.init_parameters(seed)
    _train_steps(e, steps, seed)
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def engine():
    return _engine()


def _recordings(n, seed=11, length=L):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((rng.standard_normal((length, 12)) * (1 + 0.2 * i) * 2e-3).astype(np.float32)).cuda()
            for i in range(n)]


@pytest.fixture(scope="module")
def norm():
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rec = _recordings(1, seed=5)[0]
    w = preprocess_segments(rec[None], keep=20 * np.arange(140))[0]
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
    pushes.append(left.copy())                     # the rest in one push
    return pushes


def _run_multi(dec, recs, pushes, streams=None):
    streams = range(len(recs)) if streams is None else streams
    pos = np.zeros(len(recs), dtype=np.int64)
    got = {s: [] for s in streams}
    for n in pushes:
        chunks = [None] * dec.n_streams
        for s in range(len(recs)):
            if n[s] or s % 2:                      # idle streams as None and as empty tensors
                chunks[s] = recs[s][pos[s]:pos[s] + n[s]]
        out = dec.push(chunks, return_logits=True, return_windows=True)
        for s in streams:
            got[s].append(out[s])
        pos += n
    return {s: [torch.cat([o[i] for o in got[s]]) for i in range(4)] for s in streams}


def _run_single(dec, rec, sizes):
    outs, p = [], 0
    for n in sizes:
        outs.append(dec.push(rec[p:p + n], return_logits=True, return_windows=True))
        p += n
    return [torch.cat([o[i] for o in outs]) for i in range(4)]


def _assert_same(got, ref, what):
    assert got[0].shape[0] > 0, what
    for i, name in enumerate(("pred", "voted", "logits", "windows")):
        assert got[i].shape == ref[i].shape, (what, name, got[i].shape, ref[i].shape)
        assert torch.equal(got[i], ref[i]), (what, name)


TABLES = [dict(classes=list(range(41))), dict(classes=[30, 2, 17, 5, 9]), dict(classes=[7]), dict(table="rand", k=12, ids="perm"),
          dict(classes=list(range(0, 41, 3))), dict(table="rand", k=64, ids=None), dict(classes=[40, 0])]


def _set(dec, s, spec, single=False, gen=None):
    if "classes" in spec:
        args = dict(classes=spec["classes"])
    else:
        g = torch.Generator().manual_seed(100 + s)
        t = torch.randn(spec["k"], 16, generator=g)
        ids = None if spec["ids"] is None else (torch.randperm(64, generator=g)[:spec["k"]] + 3).tolist()
        args = dict(table=t, ids=ids)
    if single:
        dec.set_classes(**args)
    else:
        dec.set_classes(s, **args)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_streams_bit_identical_to_single_stream_decoders(engine, norm, dtype):
    from contrastiveprosthetics_amd import MultiStreamDecoder, OnlineDecoder
    mean, std = norm
    S = len(TABLES)
    recs = _recordings(S)
    dec = MultiStreamDecoder(engine, mean, std, S, dtype=dtype)
    for s, spec in enumerate(TABLES):
        _set(dec, s, spec)
    pushes = _schedule(S, 20, seed=1 if dtype == "f32" else 2)
    got = _run_multi(dec, recs, pushes)
    assert list(dec.n_seen) == [L] * S
    for s, spec in enumerate(TABLES):
        ref = OnlineDecoder(engine, mean, std, dtype=dtype)
        _set(ref, s, spec, single=True)
        _assert_same(got[s], _run_single(ref, recs[s], [int(n[s]) for n in pushes]), (dtype, s))


def test_glove_tables_bit_identical(norm):
    from contrastiveprosthetics_amd import MultiStreamDecoder, OnlineDecoder
    mean, std = norm
    e = _engine(seed=4, class_encoder="glove")
    S = 3
    recs = _recordings(S, seed=12)
    rows = [torch.randn(k, 20, generator=torch.Generator().manual_seed(8 + k)) for k in (12, 3, 41)]
    dec = MultiStreamDecoder(e, mean, std, S)
    for s in range(S):
        dec.set_classes(s, glove=rows[s])
    pushes = _schedule(S, 12, seed=3)
    got = _run_multi(dec, recs, pushes)
    for s in range(S):
        ref = OnlineDecoder(e, mean, std)
        ref.set_classes(glove=rows[s])
        _assert_same(got[s], _run_single(ref, recs[s], [int(n[s]) for n in pushes]), ("glove", s))


def test_stream_isolation(engine, norm):
    from contrastiveprosthetics_amd import MultiStreamDecoder
    mean, std = norm
    recs = _recordings(256, seed=21, length=600)
    alone = MultiStreamDecoder(engine, mean, std, 256, max_rows=256 * 4)
    crowd = MultiStreamDecoder(engine, mean, std, 256, max_rows=256 * 4)
    for d in (alone, crowd):
        for s in range(256):
            d.set_classes(s, classes=list(range(41)) if s % 3 else [1, 5, 7, 30])
    A = 77
    for p in range(0, 600, 60):                         # 3 windows per push
        solo = [None] * 256
        solo[A] = recs[A][p:p + 60]
        a = alone.push(solo, return_logits=True, return_windows=True)[A]
        c = crowd.push([r[p:p + 60] for r in recs], return_logits=True, return_windows=True)[A]
        assert all(torch.equal(x, y) for x, y in zip(a, c)), p
    # reset and set_classes of some streams leave the filter and vote state of the others alone
    S = 4
    recs = _recordings(S, seed=22)
    d1 = MultiStreamDecoder(engine, mean, std, S, vote=9)
    d2 = MultiStreamDecoder(engine, mean, std, S, vote=9)
    for d in (d1, d2):
        for s in range(S):
            d.set_classes(s, classes=list(range(41)))
    first = [r[:1234] for r in recs]
    d1.push(first)
    d2.push(first)
    d1.reset(streams=[1])
    d1.set_classes(2, classes=[3, 4, 5])
    assert list(d1.n_seen) == [1234, 0, 1234, 1234]
    nxt = [r[1234:2000] for r in recs]
    o1 = d1.push(nxt, return_logits=True, return_windows=True)
    o2 = d2.push(nxt, return_logits=True, return_windows=True)
    for s in (0, 3):
        assert all(torch.equal(x, y) for x, y in zip(o1[s], o2[s])), s
    assert not torch.equal(o1[1][3], o2[1][3])         # stream 1 started over: its windows differ
    assert set(o1[2][0].tolist()) <= {3, 4, 5}


def test_scale_and_host_split(engine, norm):
    from contrastiveprosthetics_amd import MultiStreamDecoder, OnlineDecoder
    mean, std = norm
    # 256 streams, one window each per tick
    S = 256
    recs = _recordings(S, seed=31, length=200)
    dec = MultiStreamDecoder(engine, mean, std, S, dtype="bf16")
    for s in range(S):
        dec.set_classes(s, classes=[s % 41, (s * 7 + 3) % 41, 40 - s % 41] if s % 41 not in (20,) else [20])
    outs = {s: [] for s in range(S)}
    for p in range(0, 200, 20):
        res = dec.push([r[p:p + 20] for r in recs], return_logits=True, return_windows=True)
        for s in range(S):
            assert res[s][0].shape[0] == 1
            outs[s].append(res[s])
    for s in (0, 1, 100, 211, 255):
        ref = OnlineDecoder(engine, mean, std, dtype="bf16")
        ref.set_classes(classes=[s % 41, (s * 7 + 3) % 41, 40 - s % 41] if s % 41 not in (20,) else [20])
        got = [torch.cat([o[i] for o in outs[s]]) for i in range(4)]
        _assert_same(got, _run_single(ref, recs[s], [20] * 10), ("256", s))
    # a push above max_rows (and above max_windows_per_push for one stream) is split on the host
    S = 7
    recs = _recordings(S, seed=32)
    small = MultiStreamDecoder(engine, mean, std, S, max_windows_per_push=16, max_rows=40)
    for s, spec in enumerate(TABLES):
        _set(small, s, spec)
    pushes = _schedule(S, 4, seed=5, idle=0.2, hi=900)
    got = _run_multi(small, recs, pushes)
    for s, spec in enumerate(TABLES):
        ref = OnlineDecoder(engine, mean, std)
        _set(ref, s, spec, single=True)
        _assert_same(got[s], _run_single(ref, recs[s], [int(n[s]) for n in pushes]), ("split", s))
    # push_packed: the same values from a packed buffer
    packed = MultiStreamDecoder(engine, mean, std, S, max_windows_per_push=16, max_rows=40)
    for s, spec in enumerate(TABLES):
        _set(packed, s, spec)
    pos = np.zeros(S, dtype=np.int64)
    acc = {s: [] for s in range(S)}
    for n in pushes:
        raw = torch.cat([recs[s][pos[s]:pos[s] + n[s]] for s in range(S)])
        for s, o in enumerate(packed.push_packed(raw, n, return_logits=True, return_windows=True)):
            acc[s].append(o)
        pos += n
    for s in range(S):
        _assert_same([torch.cat([o[i] for o in acc[s]]) for i in range(4)], got[s], ("packed", s))


def test_refresh_matches_online_decoder(norm):
    from contrastiveprosthetics_amd import MultiStreamDecoder, OnlineDecoder
    mean, std = norm
    e = _engine(seed=6)
    recs = _recordings(3, seed=41)
    dec = MultiStreamDecoder(e, mean, std, 3)
    for s in range(3):
        dec.set_classes(s, classes=list(range(41)) if s != 1 else [4, 8, 15, 16, 23])
    dec.set_classes(2, table=torch.randn(6, 16, generator=torch.Generator().manual_seed(1)))
    a = dec.push([r[:1500] for r in recs], return_logits=True)
    _train_steps(e, 1, 99)
    dec.reset()
    b = dec.push([r[:1500] for r in recs], return_logits=True)
    for s in range(3):
        assert all(torch.equal(x, y) for x, y in zip(a[s], b[s]))       # still the folded copy
    dec.refresh()
    dec.reset()
    c = dec.push([r[:1500] for r in recs], return_logits=True)
    for s in range(3):
        ref = OnlineDecoder(e, mean, std)
        if s == 2:
            ref.set_classes(table=torch.randn(6, 16, generator=torch.Generator().manual_seed(1)))
        else:
            ref.set_classes(list(range(41)) if s != 1 else [4, 8, 15, 16, 23])
        ref.refresh()
        r = ref.push(recs[s][:1500], return_logits=True)
        assert all(torch.equal(x, y) for x, y in zip(c[s], r)), s
        assert not torch.equal(c[s][2], a[s][2])


def test_refusals(engine, norm):
    from contrastiveprosthetics_amd import MultiStreamDecoder, OnlineDecoder, _lib
    from contrastiveprosthetics_amd.engine import Engine
    mean, std = norm
    ada = Engine(adabn=True, dtype="f32", device="cuda:0")
    with pytest.raises(_lib.CpNativeError, match="AdaBN"):
        MultiStreamDecoder(ada, mean, std, 2)
    with pytest.raises(_lib.CpNativeError, match="adapt"):
        MultiStreamDecoder(engine, mean, std, 2, adapt=0.01)
    with pytest.raises(_lib.CpNativeError, match="8-bit"):
        MultiStreamDecoder(engine, mean, std, 2, dtype="fp8")
    for bad in (0, 257):
        with pytest.raises(ValueError, match="n_streams"):
            MultiStreamDecoder(engine, mean, std, bad)
    with pytest.raises(ValueError, match="max_rows"):
        MultiStreamDecoder(engine, mean, std, 2, max_rows=0)
    recs = _recordings(3, seed=51)
    d = MultiStreamDecoder(engine, mean, std, 3)
    ref = MultiStreamDecoder(engine, mean, std, 3)
    for x in (d, ref):
        x.set_classes(0, classes=list(range(41)))
        x.set_classes(2, classes=[1, 2, 3])
    for bad in (3, -1, 1.0):
        with pytest.raises(IndexError):
            d.set_classes(bad, classes=[1])
        with pytest.raises(IndexError):
            d.reset(streams=[0, bad])
    with pytest.raises(ValueError, match="at most 64"):
        d.set_classes(0, table=torch.randn(65, 16))
    with pytest.raises(ValueError, match="empty"):
        d.set_classes(0, classes=[])
    with pytest.raises(_lib.CpNativeError, match="no class table"):
        d.push([recs[0][:100], recs[1][:100], None])
    for chunks in ([recs[0][:100]], [recs[0][:100].cpu(), None, None], [recs[0][:100].double(), None, None],
                   [recs[0][:100, :6], None, None], recs[0][:300].reshape(3, 100, 12)):
        with pytest.raises(ValueError):
            d.push(chunks)
    with pytest.raises(ValueError, match="counts"):
        d.push_packed(recs[0][:100], [50, 0, 40])
    with pytest.raises(ValueError, match="counts"):
        d.push_packed(recs[0][:100], [100, 0])
    assert list(d.n_seen) == [0, 0, 0]
    # nothing was enqueued by the refusals: the decoder computes what an untouched one does
    chunks = [recs[0][:700], None, recs[2][:500]]
    o, r = d.push(chunks, return_logits=True), ref.push(chunks, return_logits=True)
    for s in (0, 2):
        assert all(torch.equal(x, y) for x, y in zip(o[s], r[s]))
    single = OnlineDecoder(engine, mean, std, classes=[1, 2, 3])
    assert all(torch.equal(x, y) for x, y in zip(o[2], single.push(recs[2][:500], return_logits=True)))
