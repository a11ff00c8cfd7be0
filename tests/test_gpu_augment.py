"""The gather augmentation on the device (cp_gather_groups_aug) against augment.Augment.reference, the numpy
definition: exact where the perturbation is a permutation or a fill, within 16 * 2^-24 * A of the float64 chain where it is
arithmetic, independent of the launch, reproducible as a stream, identical under graph replay, and wired through TaskWrapper,
results.robustness and train.py.

The table is 41 x 40 rows with x[row][ch] = row + ch / 16 (exact in f32): a wrong row or channel shows in the value itself."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, D = 41, 40
U = 2.0 ** -24
BEST = dict(d_e=16, lr_emg=9.761e-4, reg_emg=7.103e-5, dp_emg=0.0, lr_glove=2.653e-3, reg_glove=2.840e-6, dp_glove=0.0)
MEAN_STD = np.concatenate([np.linspace(5, 60, 12), np.linspace(1, 9, 12)]).astype(np.float32)


@pytest.fixture(scope="module")
def data():
    """table (1640, 12); V = 1: emg_rand (41, 40) of row indices, V = 25: (41, 8) of indices of 25-row items; perm (7,)"""
    g = torch.Generator().manual_seed(3)
    table = (torch.arange(T * D, dtype=torch.float32).reshape(-1, 1) + torch.arange(12, dtype=torch.float32) / 16).cuda()
    rand1 = (torch.rand(T, D, generator=g).argsort(-1) + torch.arange(T).reshape(T, 1) * D).cuda()
    rand25 = torch.randint(0, T * D // 25, (T, 8), generator=g).cuda()
    perm = torch.tensor([5, 0, 7, 2, 6, 1, 3]).cuda()
    return table, {1: rand1, 25: rand25}, perm


def plain(data, B, V):
    from contrastiveprosthetics_amd import engine as E
    table, rand, perm = data
    return E.gather_groups(table, rand[V], perm[:B], V)


def aug_gather(data, aug, B, V, item_offset=0, first=0):
    from contrastiveprosthetics_amd import engine as E
    table, rand, perm = data
    return E.gather_groups(table, rand[V], perm[first:first + B], V, augment=aug, item_offset=item_offset)


def raw_call(data, B, V, struct, rand=None):
    """cp_gather_groups_aug with a cp_augment built by hand (an all-off one never reaches the entry through Engine.gather)"""
    from contrastiveprosthetics_amd import _lib
    table, rands, perm = data
    rand = rands[V] if rand is None else rand
    out = torch.empty(B, T, V, 12, device="cuda")
    _lib.check(_lib.load().cp_gather_groups_aug(table.data_ptr(), table.shape[0], rand.data_ptr(), rand.shape[1], perm.data_ptr(),
                                                B, V, out.data_ptr(), C.byref(struct), torch.cuda.current_stream().cuda_stream),
               "cp_gather_groups_aug")
    return out


@pytest.mark.parametrize("B,V", [(1, 1), (7, 1), (1, 25), (7, 25)])
def test_everything_off_is_the_plain_gather(data, B, V):
    from contrastiveprosthetics_amd import engine as E
    from contrastiveprosthetics_amd.augment import Augment
    table, rand, perm = data
    want = plain(data, B, V)
    assert torch.equal(want.reshape(-1, 12), table[(rand[V][:, perm[:B]].t().reshape(-1, 1) * V + torch.arange(V).cuda()).reshape(-1)])
    off = Augment(fill=3.0, mean_std=MEAN_STD, seed=9)
    e = E.Engine(adabn=True, dtype="f32", device="cuda")
    assert torch.equal(e.gather(table, rand[V], perm[:B], V, augment=off), want) and off.count == 0
    assert torch.equal(E.gather_groups(table, rand[V], perm[:B], V, augment=off), want)
    assert torch.equal(raw_call(data, B, V, off.struct(77, device="cuda")), want)            # the new kernel itself
    assert torch.equal(raw_call(data, B, V, Augment().struct(1, item_offset=2 ** 31)), want)


def test_rows_outside_the_table_are_still_counted(data):
    from contrastiveprosthetics_amd import engine as E
    from contrastiveprosthetics_amd.augment import Augment
    table, rand, perm = data
    bad = rand[1].clone()
    bad[3, 2] = T * D + 5
    bad[7, 0] = -1
    E.gather_oob_count(reset=True)
    out = raw_call(data, 7, 1, Augment(shift=1).struct(1), rand=bad)
    assert E.gather_oob_count(reset=True) == 2 and E.gather_oob_count(reset=False) == 0
    from contrastiveprosthetics_amd.online import rotations
    rot = torch.from_numpy(rotations()[1].astype(np.int64)).cuda()
    b_of = {int(p): b for b, p in enumerate(perm.tolist())}
    assert torch.equal(out[b_of[2], 3, 0], table[0][rot]) and torch.equal(out[b_of[0], 7, 0], table[0][rot])     # read from row 0
    aug_gather(data, Augment(shift=1), 7, 1)
    assert E.gather_oob_count(reset=True) == 0


@pytest.mark.parametrize("V", [1, 25])
def test_shift_and_dead_channels_are_exact(data, V):
    from contrastiveprosthetics_amd.augment import Augment, salt_of
    from contrastiveprosthetics_amd.online import rotations
    B = 7
    want = plain(data, B, V)
    for s in (-7, -1, 1, 3):
        got = aug_gather(data, Augment(shift=s), B, V)
        assert torch.equal(got, want[..., torch.from_numpy(rotations()[s % 8].astype(np.int64)).cuda()]), s
    # a shift drawn per item: the reference's maps, exactly
    a = Augment(shift=(-3, 3), seed=11)
    got = aug_gather(data, a, B, V).reshape(-1, 12).cpu().numpy()
    ref, parts = a.reference(want.reshape(-1, 12).cpu().numpy(), 0, V, salt_of(1), parts=True)
    assert a.count == 1 and np.array_equal(got.astype(np.float64), ref)
    shifts = parts["shift"].reshape(B * T, V)
    assert (shifts == shifts[:, :1]).all() and len(set(shifts[:, 0].tolist())) == 7       # one per item, every value of -3..3 drawn
    # dead electrodes: the fill there, everything else untouched
    got = aug_gather(data, Augment(dead=(0, 11), fill=-2.5), B, V)
    assert (got[..., [0, 11]] == -2.5).all() and torch.equal(got[..., 1:11], want[..., 1:11])
    assert (aug_gather(data, Augment(p_drop=1.0, fill=0.25), B, V) == 0.25).all()
    a = Augment(p_drop=0.3, seed=5)
    got = aug_gather(data, a, B, V).reshape(-1, 12).cpu().numpy()
    ref, parts = a.reference(want.reshape(-1, 12).cpu().numpy(), 0, V, salt_of(1), parts=True)
    assert np.array_equal(got.astype(np.float64), ref)
    dead = parts["dead"].reshape(B * T, V, 12)
    assert (dead == dead[:, :1]).all() and 0.2 < dead.mean() < 0.4                       # one dead set per item


def chain_bound(x, parts, aug):
    """16 * 2^-24 * A per element: A = ((|x_c std_c| + |mean_c|) G + |mean_d|) / std_d + |noise|, without mean_std |x_c| G + |noise|"""
    c, G, noise = parts["c"], parts["G"], np.abs(parts["noise"])
    xc = np.abs(np.take_along_axis(x.astype(np.float64), c, axis=1))
    if aug.mean_std is None:
        return 16 * U * (xc * G + noise)
    m, sd = np.abs(aug.mean_std[:12].astype(np.float64)), aug.mean_std[12:].astype(np.float64)
    return 16 * U * (((xc * sd[c] + m[c]) * G + m[None, :]) / sd[None, :] + noise)


WORST = {}


@pytest.mark.parametrize("item_offset", [0, 2 ** 31 + 5])
@pytest.mark.parametrize("B,V", [(7, 1), (3, 25)])
@pytest.mark.parametrize("with_mean_std", [True, False])
def test_full_chain_against_the_float64_reference(data, with_mean_std, B, V, item_offset):
    """Everything on.  Largest observed error / (2^-24 A) on the MI355X over the eight cases: 4.40 (bound 16)."""
    from contrastiveprosthetics_amd.augment import Augment, salt_of
    x = plain(data, B, V).reshape(-1, 12).cpu().numpy()
    a = Augment(shift=(-3, 3), p_drop=0.15, dead=(9,), gain_sigma=0.35, amp_sigma=0.2, noise_sigma=0.05, fill=-0.5,
                mean_std=MEAN_STD if with_mean_std else None, seed=21)
    got = aug_gather(data, a, B, V, item_offset=item_offset).reshape(-1, 12).cpu().numpy().astype(np.float64)
    ref, parts = a.reference(x, item_offset, V, salt_of(1), parts=True)
    bound = chain_bound(x, parts, a)
    err = np.abs(got - ref)
    live = ~parts["dead"]
    ratio = float((err[live] / (bound[live] / 16)).max())
    WORST[(with_mean_std, B, V, item_offset)] = ratio
    print(f"mean_std={with_mean_std} B={B} V={V} item_offset={item_offset}: max error / (2^-24 A) = {ratio:.3f}; "
          f"largest so far {max(WORST.values()):.3f}")
    assert np.array_equal(got[~live], ref[~live]) and (ref[~live] == -0.5).all() and 0.1 < (~live).mean() < 0.4
    assert (err[live] <= bound[live]).all(), ratio
    assert np.abs(got - x)[live].max() > 0.05                      # (something was perturbed)


@pytest.mark.parametrize("V", [1, 25])
def test_unchanged_channels_keep_their_bits_under_mean_std(data, V):
    """With mean_std a channel that keeps its source (c == d) and has no gain (G == 1) is x[d] itself, not a round trip through
    the raw value; the channels that moved are renormalised with the model channel's constants."""
    from contrastiveprosthetics_amd.augment import Augment, salt_of
    B = 3
    x = plain(data, B, V).reshape(-1, 12).cpu().numpy()
    a = Augment(shift=(-3, 3), mean_std=MEAN_STD, seed=2)
    got = aug_gather(data, a, B, V).reshape(-1, 12).cpu().numpy()
    ref, parts = a.reference(x, 0, V, salt_of(1), parts=True)
    same = parts["c"] == np.arange(12)[None, :]
    assert np.array_equal(got[same], x[same]) and same[:, 8:].all() and 0.3 < same.mean() < 0.6
    assert not np.array_equal(got[~same], np.take_along_axis(x, parts["c"], 1)[~same])
    assert (np.abs(got - ref) <= chain_bound(x, parts, a)).all()
    # noise on top: the unchanged channels are x[d] + noise, one f32 addition
    a = Augment(noise_sigma=0.05, mean_std=MEAN_STD, seed=2)
    got = aug_gather(data, a, B, V).reshape(-1, 12).cpu().numpy()
    _, parts = a.reference(x, 0, V, salt_of(1), parts=True)
    sig = np.float32(a.noise_sigma)
    n32 = a.draws(0, B * T, V, salt_of(1))["n_noise"].reshape(-1, 12)
    assert np.array_equal(got, x + sig * n32)


def test_an_item_does_not_depend_on_the_launch(data):
    from contrastiveprosthetics_amd.augment import Augment
    kw = dict(shift=(-3, 3), p_drop=0.15, gain_sigma=0.35, amp_sigma=0.2, noise_sigma=0.05, mean_std=MEAN_STD, seed=8)
    for V in (1, 25):
        whole = aug_gather(data, Augment(**kw), 7, V)
        part = aug_gather(data, Augment(**kw), 2, V, item_offset=T * 3, first=3)
        assert torch.equal(whole[3:5], part), V
        assert not torch.equal(aug_gather(data, Augment(**kw), 2, V, item_offset=0, first=3), part)


def test_stream_of_gathers(data):
    from contrastiveprosthetics_amd.augment import Augment
    kw = dict(shift=(-3, 3), gain_sigma=0.3, noise_sigma=0.05)
    a, b, c = Augment(seed=4, **kw), Augment(seed=4, **kw), Augment(seed=5, **kw)
    a1, a2 = aug_gather(data, a, 7, 1), aug_gather(data, a, 7, 1)
    b1, b2 = aug_gather(data, b, 7, 1), aug_gather(data, b, 7, 1)
    c1 = aug_gather(data, c, 7, 1)
    assert (a.count, b.count, c.count) == (2, 2, 1)
    assert not torch.equal(a1, a2) and torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, c1)


def step_data(Dn=500, seed=5):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(T, 1, 12, generator=g)
    table = (mu + torch.randn(T, Dn, 12, generator=g)).reshape(T * Dn, 12).cuda()
    emg_rand = (torch.rand(T, Dn, generator=g).argsort(-1) + torch.arange(T).reshape(T, 1) * Dn).cuda()
    perms = [torch.randperm(Dn, generator=g)[:8].cuda() for _ in range(6)]
    return table, emg_rand, perms


@pytest.mark.parametrize("dtype,adabn", [("f32", False), ("bf16", True)])
def test_graph_step_with_augmentation_equals_eager_steps(dtype, adabn):
    from contrastiveprosthetics_amd.augment import Augment
    from contrastiveprosthetics_amd.engine import Engine, GraphStep
    table, emg_rand, perms = step_data()
    labels = torch.arange(T).repeat(8).cuda()
    runs = []
    for mode in ("eager", "graph"):
        e = Engine(adabn=adabn, dtype=dtype, dp_emg=0.0, device="cuda", seed=3)
        e.init_parameters(11)
        aug = Augment(shift=1, gain_sigma=0.3, p_drop=0.1, seed=6)
        losses = []
        if mode == "graph":
            gs = GraphStep(e, table, emg_rand, 8, BEST, augment=aug)
            assert aug.count == 0                                   # warm-up and capture drew nothing from the stream
            for perm in perms:
                losses.append(gs.step(perm)[0].item())
        else:
            for perm in perms:
                x = e.gather(table, emg_rand, perm, 1, augment=aug)
                z = e.encoder_forward(x, training=True)
                out, _, _ = e.head(z, labels, 1, want_grad=True)
                e.encoder_backward(x)
                e.adam_step(BEST)
                losses.append(out[0].item())
        torch.cuda.synchronize()
        runs.append((e, losses, aug.count))
    (a, la, ca), (b, lb, cb) = runs
    assert ca == cb == 6 and la == lb
    assert torch.equal(a.values.flat, b.values.flat)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    # and the augmentation is in it: the same steps without one end elsewhere
    e = Engine(adabn=adabn, dtype=dtype, dp_emg=0.0, device="cuda", seed=3)
    e.init_parameters(11)
    x = e.gather(table, emg_rand, perms[0], 1)
    z = e.encoder_forward(x, training=True)
    out, _, _ = e.head(z, labels, 1, want_grad=True)
    assert out[0].item() != la[0]


def test_graph_replays_draw_a_new_perturbation_each(data):
    from contrastiveprosthetics_amd.augment import Augment
    from contrastiveprosthetics_amd.engine import Engine, GraphStep
    table, emg_rand, perms = step_data()
    e = Engine(adabn=True, dtype="f32", dp_emg=0.0, device="cuda", seed=3)
    e.init_parameters(11)
    frozen = dict(BEST, lr_emg=0.0, lr_glove=0.0, reg_emg=0.0, reg_glove=0.0)
    gs = GraphStep(e, table, emg_rand, 8, frozen, augment=Augment(shift=1, gain_sigma=0.3, p_drop=0.1, seed=6))
    w0 = e.values.flat.clone()
    losses = [gs.step(perms[0])[0].item() for _ in range(3)]       # one perm, frozen weights: only the draws can change
    assert torch.equal(e.values.flat, w0)
    assert len(set(losses)) == 3, losses


@pytest.fixture(scope="module")
def wrapped():
    from contrastiveprosthetics_amd.load import DB23
    from contrastiveprosthetics_amd.utils import TaskWrapper
    ds = DB23()
    ds.load_synthetic()
    return TaskWrapper(ds)


def test_taskwrapper_augments_in_train_mode_and_perturbs_in_eval_mode(wrapped):
    from contrastiveprosthetics_amd.augment import Augment
    from contrastiveprosthetics_amd.online import rotations
    ds = wrapped
    assert ds.augment is None and ds.perturb is None
    rot1 = torch.from_numpy(rotations()[1].astype(np.int64)).cuda()
    rot2 = torch.from_numpy(rotations()[2].astype(np.int64)).cuda()
    perm = torch.arange(5).cuda()
    try:
        for mode, V in (("train", 1), ("val", 25), ("test", 25)):
            getattr(ds, "set_" + mode)()
            ds.augment = ds.perturb = None
            base = ds.batch(perm)[0]
            assert base.shape == (5, T, V, 1, 12)
            ds.augment, ds.perturb = Augment(shift=1), Augment(shift=2)
            got = ds.batch(perm)[0]
            assert torch.equal(got, base[..., rot1 if mode == "train" else rot2]), mode
            assert (ds.augment.count, ds.perturb.count) == ((1, 0) if mode == "train" else (0, 1))
            ds.augment, ds.perturb = (None, Augment(shift=2)) if mode == "train" else (Augment(shift=1), None)
            assert torch.equal(ds.batch(perm)[0], base), mode          # the other mode's setting is not applied
    finally:
        ds.augment = ds.perturb = None


def test_robustness_table_of_a_fresh_model(wrapped, tmp_path):
    from contrastiveprosthetics_amd import results
    from contrastiveprosthetics_amd.models import Model
    from contrastiveprosthetics_amd.online import rotations
    ds = wrapped
    results.args = results.build_parser().parse_args(["--batch_size", "8", "--synthetic", "--dtype", "bf16",
                                                      "--save", str(tmp_path) + "/"])
    params = dict(BEST, epochs=1)
    # AdaBN (the CLI's default): evaluation normalises with the batch's statistics, so every comparison below runs the same
    # batches -- one seed, hence one sampler table and one order, per pass
    model = Model(params=params, train_model=True, adabn=True, dtype="bf16").to(torch.float32)
    try:
        torch.manual_seed(5)
        loss, acc = results.test(model, ds, save=str(tmp_path) + "/")
        torch.manual_seed(5)
        table = results.robustness(model, ds)
        assert table.shape == (7, 13, 2) and ds.perturb is None
        assert table[3, 0, 1] == acc                                  # (shift 0, dead None) is the plain test pass
        assert ((table >= 0) & (table <= 1)).all()
        print("distinct per-window accuracies in the table:", len(np.unique(table[..., 0])))
        # a shift-s row is the evaluation of the table whose ring columns were turned by s
        for i, s in ((1, -2), (6, 3)):
            torch.manual_seed(5)
            ds.set_test()
            order = torch.randperm(len(ds)).to(ds.device)
            ds.dataset.EMG_use = ds.dataset.EMG_use[:, torch.from_numpy(rotations()[s % 8].astype(np.int64)).cuda()].contiguous()
            model.set_test()
            hits, windows = 0.0, 0
            for k in range(0, len(ds), 8):
                EMG, GLOVE, label = ds.batch(order[k:k + 8])
                with torch.no_grad():
                    logits = model.forward(EMG, GLOVE, label.reshape(-1))
                    model.loss(logits, label.reshape(-1))
                hits += float(model._pending["out"][1].item())
                windows += logits.shape[0] * T
            assert table[i, 0, 0] == hits / windows and table[i, 0, 1] == model.correct(), s
    finally:
        results.args = None
        ds.set_test()


def test_train_cli_with_augmentation_graph_equals_eager(tmp_path):
    from contrastiveprosthetics_amd import train
    cks = []
    for mode in ("eager", "graph"):
        d = tmp_path / mode
        (d / "data").mkdir(parents=True)
        np.save(d / "data" / "cross_val_values.npy", np.array([[3.2, 0.25]]))
        np.save(d / "data" / "cross_val_keys.npy", np.array([[16, 9.761e-4, 7.103e-5, 0.0, 2.653e-3, 2.840e-6, 0.0]]))
        argv = ["--final_epochs=1", "--batch_size=16", "--crossval_load", "--synthetic", "--dtype", "bf16", "--aug_shift", "1",
                "--aug_gain", "0.2", "--data_dir", str(d / "data"), "--checkpoint_dir", str(d / "ckpt")]
        if mode == "graph":
            argv.append("--graph")
        train.main(train.build_parser().parse_args(argv))
        cks.append(torch.load(d / "ckpt" / "contrastive.pt", weights_only=True))
    a, b = cks
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # and the flags did something: the same epoch without them ends elsewhere
    d = tmp_path / "plain"
    (d / "data").mkdir(parents=True)
    np.save(d / "data" / "cross_val_values.npy", np.array([[3.2, 0.25]]))
    np.save(d / "data" / "cross_val_keys.npy", np.array([[16, 9.761e-4, 7.103e-5, 0.0, 2.653e-3, 2.840e-6, 0.0]]))
    train.main(train.build_parser().parse_args(["--final_epochs=1", "--batch_size=16", "--crossval_load", "--synthetic", "--dtype",
                                                "bf16", "--data_dir", str(d / "data"), "--checkpoint_dir", str(d / "ckpt")]))
    c = torch.load(d / "ckpt" / "contrastive.pt", weights_only=True)
    assert not torch.equal(a["emg_net.linear.0.weight"], c["emg_net.linear.0.weight"])
