"""The online decoder on the MI355X (contrastiveprosthetics_amd/online.py, csrc/online.cuh): front end bit-identical to the
offline preprocessing, chunk invariance, agreement with the eval path of the engine, subsets, the vote ring, glove class
tables, refresh() and refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 5130
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
    e = _engine()
    rm = e.running["emg_net.linear.23.running_var"]
    assert float((rm - 1).abs().max()) > 1e-3                  # running statistics are not the defaults
    return e


@pytest.fixture(scope="module")
def recording():
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rng = np.random.default_rng(11)
    rec = torch.from_numpy((rng.standard_normal((L, 12)) * 2e-3).astype(np.float32)).cuda()
    w = preprocess_segments(rec[None], keep=20 * np.arange(256))[0]
    return rec, w.mean(0), w.std(0)


def _chunkings(seed=0):
    rng = np.random.default_rng(seed)
    rnd, s = [], 0
    while s < L:
        n = int(min(rng.integers(1, 400), L - s))
        rnd.append(n)
        s += n
    return {"whole": [L], "1": [1] * L, "7": None, "20": None, "333": None, "random": rnd}


def _split(c, name):
    if c is not None:
        return c
    n = int(name)
    return [n] * (L // n) + ([L % n] if L % n else [])


def _run(dec, rec, chunks):
    outs, s = [], 0
    for n in chunks:
        outs.append(dec.push(rec[s:s + n], return_logits=True, return_windows=True))
        s += n
    return [torch.cat([o[i] for o in outs]) for i in range(4)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("phase", [0, 13])
def test_front_end_bit_identical_and_chunk_invariant(engine, recording, dtype, phase):
    from contrastiveprosthetics_amd import OnlineDecoder
    from contrastiveprosthetics_amd.preprocess import normalize_, preprocess_segments
    rec, mean, std = recording
    K = (L - phase + 9) // 20
    ref = normalize_(preprocess_segments(rec[None], keep=phase + 20 * np.arange(K)), mean, std)[0]
    dec = OnlineDecoder(engine, mean, std, classes=list(range(41)), dtype=dtype, phase=phase)
    base = None
    for name, c in _chunkings(phase).items():
        dec.reset()
        pred, voted, logits, win = _run(dec, rec, _split(c, name))
        assert win.shape == ref.shape, name
        assert torch.equal(win, ref), (name, float((win - ref).abs().max()))
        if base is None:
            base = (pred, voted, logits)
        else:
            assert torch.equal(pred, base[0]) and torch.equal(voted, base[1]) and torch.equal(logits, base[2]), name


def _ref_logits(engine, windows, table):
    n = windows.shape[0]
    x = torch.zeros((n + 40) // 41 * 41, 12, device=windows.device)        # the encoder takes whole groups of 41 rows
    x[:n] = windows
    z = engine.encoder_forward(x, training=False)[:n]
    zn = z / z.norm(dim=-1, keepdim=True)
    tn = table / table.norm(dim=-1, keepdim=True)
    return zn @ tn.t()


def test_against_the_eval_path(engine, recording):
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    d32 = OnlineDecoder(engine, mean, std, classes=list(range(41)), dtype="f32")
    p32, v32, l32, win = d32.push(rec, return_logits=True, return_windows=True)
    table = (engine.values.views["glove_net.easy.0.weight"].t() + engine.values.views["glove_net.easy.0.bias"])
    ref = _ref_logits(engine, win, table)
    dev = float((l32 - ref).abs().max())
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    print(f"f32 decoder vs encoder_forward(eval): max |logit diff| {dev:.3e} over {l32.shape[0]} windows")
    assert dev <= 1e-4
    assert torch.equal(p32[clear].long(), ref.argmax(1)[clear])
    d16 = OnlineDecoder(engine, mean, std, classes=list(range(41)), dtype="bf16")
    p16, v16, l16 = d16.push(rec, return_logits=True)
    dev16 = float((l16 - l32).abs().max())
    agree = float((p16 == p32).float().mean())
    gap = (l32.topk(2, dim=1).values[:, 0] - l32.topk(2, dim=1).values[:, 1])
    print(f"bf16 decoder vs f32 decoder: max |logit diff| {dev16:.3e}, argmax agreement {agree:.4f}, "
          f"min top-2 gap of the disagreeing windows {float(gap[p16 != p32].max()) if (p16 != p32).any() else 0:.3e}")
    assert dev16 <= 2e-2
    assert agree >= 0.99


def test_subset_prediction(engine, recording):
    from contrastiveprosthetics_amd import OnlineDecoder
    from oracle.eval_cpu import subset_predict
    rec, mean, std = recording
    full = OnlineDecoder(engine, mean, std, classes=list(range(41)))
    _, _, l41 = full.push(rec, return_logits=True)
    rng = np.random.default_rng(2)
    ids = rng.choice(41, size=9, replace=False)                 # unsorted on purpose
    sub = OnlineDecoder(engine, mean, std, classes=ids)
    pred, _, lsub = sub.push(rec, return_logits=True)
    mask = np.zeros(41, dtype=bool)
    mask[ids] = True
    l = l41.cpu().numpy()
    ref = subset_predict(np.repeat(l[:, None, :], 41, axis=1), mask)[:, int(ids[0])]
    assert np.array_equal(pred.cpu().numpy(), ref)
    assert torch.equal(lsub, l41[:, torch.as_tensor(np.sort(ids)).cuda()])


def _trailing_modes(pred, V):
    from oracle.eval_cpu import prefix_mode
    return np.array([prefix_mode(pred[max(0, j - V + 1):j + 1])[-1] for j in range(len(pred))])


@pytest.mark.parametrize("vote", [4, 25])
def test_vote_ring(engine, recording, vote):
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    probe = OnlineDecoder(engine, mean, std, classes=list(range(41)))
    _, _, _, win = probe.push(rec, return_logits=True, return_windows=True)
    zn = _ref_logits(engine, win, torch.eye(16, device=win.device))         # z / |z|
    # two or three rows taken from the stream's own embeddings: predictions switch often, so the ring sees ties
    table = zn[[0, 101, 202][: 2 if vote == 4 else 3]].contiguous()
    dec = OnlineDecoder(engine, mean, std, vote=vote)
    dec.set_classes(table=table)
    pred, voted = dec.push(rec[:2600])
    p, v = pred.cpu().numpy(), voted.cpu().numpy()
    assert np.array_equal(v, _trailing_modes(p, vote))
    ties = 0
    for j in range(len(p)):
        c = np.bincount(p[max(0, j - vote + 1):j + 1], minlength=3)
        ties += int((c == c.max()).sum() > 1)
    assert ties > 0 and len(set(p.tolist())) > 1
    # a new class table empties the ring: the rest of the stream votes from scratch
    dec.set_classes(table=table)
    pred2, voted2 = dec.push(rec[2600:])
    p2 = pred2.cpu().numpy()
    assert np.array_equal(voted2.cpu().numpy(), _trailing_modes(p2, vote))
    assert voted2[0].item() == pred2[0].item()


def test_glove_class_table(recording):
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    e = _engine(seed=4, class_encoder="glove")
    rows = torch.randn(12, 20, generator=torch.Generator().manual_seed(8))
    dec = OnlineDecoder(e, mean, std)
    dec.set_classes(glove=rows)
    _, _, lg, win = dec.push(rec[:2000], return_logits=True, return_windows=True)
    padded = torch.zeros(41, 20)                                 # the glove encoder takes groups of 41 rows
    padded[:12] = rows
    zg = e.glove_forward(padded.cuda().reshape(1, 41, 20), training=False)[:12]
    ref = _ref_logits(e, win, zg)
    assert float((lg - ref).abs().max()) <= 1e-4
    byhand = OnlineDecoder(e, mean, std)
    byhand.set_classes(table=zg)
    _, _, lt = byhand.push(rec[:2000], return_logits=True)
    assert torch.equal(lt, lg)


def test_refresh(recording):
    from contrastiveprosthetics_amd import OnlineDecoder
    rec, mean, std = recording
    e = _engine(seed=6)
    dec = OnlineDecoder(e, mean, std, classes=list(range(41)))
    a = dec.push(rec[:1500], return_logits=True)
    _train_steps(e, 1, 99)
    dec.reset()
    b = dec.push(rec[:1500], return_logits=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))            # still the folded copy
    dec.refresh()
    dec.reset()
    c = dec.push(rec[:1500], return_logits=True)
    fresh = OnlineDecoder(e, mean, std, classes=list(range(41))).push(rec[:1500], return_logits=True)
    assert all(torch.equal(x, y) for x, y in zip(c, fresh))
    assert not torch.equal(c[2], a[2])


def test_refusals(engine, recording):
    from contrastiveprosthetics_amd import OnlineDecoder, _lib
    from contrastiveprosthetics_amd.engine import Engine
    rec, mean, std = recording
    ada = Engine(adabn=True, dtype="f32", device="cuda:0")
    with pytest.raises(_lib.CpNativeError, match="AdaBN"):
        OnlineDecoder(ada, mean, std, classes=[1, 2])
    with pytest.raises(_lib.CpNativeError, match="8-bit"):
        OnlineDecoder(engine, mean, std, classes=[1, 2], dtype="fp8")
    with pytest.raises(ValueError, match="at most 64"):
        OnlineDecoder(engine, mean, std).set_classes(table=torch.randn(65, 16))
    with pytest.raises(ValueError, match="empty"):
        OnlineDecoder(engine, mean, std, classes=[])
    # a refused set_classes enqueues nothing: the vote ring of d1 is not emptied
    d1 = OnlineDecoder(engine, mean, std, classes=list(range(41)))
    d2 = OnlineDecoder(engine, mean, std, classes=list(range(41)))
    d1.push(rec[:1000]); d2.push(rec[:1000])
    with pytest.raises(ValueError):
        d1.set_classes(table=torch.randn(65, 16))
    with pytest.raises(ValueError):
        d1.set_classes([])
    x1, x2 = d1.push(rec[1000:3000]), d2.push(rec[1000:3000])
    assert torch.equal(x1[0], x2[0]) and torch.equal(x1[1], x2[1])
    # raw that is not an (n, 12) float32 GPU tensor, a non-tensor included: the one refusal every entry point gives
    for bad in (rec[:100].cpu(), rec[:100].double(), rec[:100, :11], rec[:100].cpu().numpy(), None):
        with pytest.raises(ValueError, match="float32 tensor on the GPU"):
            d1.push(bad)
