"""The pose filter on the MI355X (contrastiveprosthetics_amd/kalman.py, csrc/online_kalman.cuh) against the numpy definitions,
in every bit, float64 words included: the moments, the design, the sweep, the stage against `FilterReference` for any cut of
the rows and any set of streams in a launch, the stage behind a push of every decoder form and of a gate, the cross-fit and
`pick_filter`'s tables."""
import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import _lib
from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import kalman as KF
from contrastiveprosthetics_amd import kinematics as K
from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, CommandGate, MultiStreamDecoder, OnlineDecoder, window_labels
from test_gpu_online_kinematics import IDS, Source, host, model, recording, stored  # noqa: F401  (recording: a fixture)
from test_gpu_online_track import _engine
from test_online_kalman_host import EVENTS, crafted_rows, filter_case, same_bits, same_f32

pytestmark = pytest.mark.gpu

F = np.float32
CUTS = [1, 16, 17, 25, None]                                   # rows per call; None: all at once
NAMES = ("raw", "filtered", "pose", "angle")


@pytest.fixture(scope="module")
def engine():
    return _engine()


def same(got, want):
    return same_f32(got, want) if want.dtype == F else same_bits(got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# moments, design and sweep against the definitions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 17, 100])
def test_moments_equal_the_definition_in_every_bit(n):
    """three groups of which group 1 is empty, an unused window in the middle of a block; 1, 2, 16, 17 and 32 joints"""
    a, y, groups, lo, span, rest = filter_case(n, 32, seed=10 + n)
    groups[groups == 1] = 2 if n >= 17 else 0
    if n < 17:
        groups[:] = 0
    else:
        assert (groups < 0).sum() == 1 and 0 < int(np.argmin(groups)) < n - 1
    for d in (1, 2, 16, 17, 32):
        ad, yd = np.ascontiguousarray(a[:, :d]), np.ascontiguousarray(y[:, :d])
        c = KF.centre(lo[:d], span[:d], rest[:d])
        want = KF.moments_reference(ad, yd, groups, 3, c)
        assert want["n"][1] == 0 and want["n"][0] >= 1 and not want["G"][1].any()
        got = KF.moments(torch.from_numpy(ad).cuda(), yd, groups, 3, c)
        assert same_bits(got["n"].cpu().numpy().astype(np.int64), want["n"]), (d, got["n"])
        for key in ("G", "C", "S", "E"):
            g = got[key].cpu().numpy()
            assert same_bits(g, want[key]), (key, d, np.abs(g - want[key]).max())


def test_an_empty_recording_and_one_without_a_counted_window_give_zero_moments():
    for n in (0, 2):
        got = KF.moments(torch.zeros(n, 3, device="cuda"), np.zeros((n, 3), F), None, 2, np.zeros(3, F))
        assert all(not got[k].cpu().numpy().any() for k in ("n", "G", "C", "S", "E"))


PLANS = [((0, 1, 2), 1e-3, 1.0, 1.0, 1), ((0, 2), 1e-3, 0.25, 4.0, 2), ((0, 1, 2), 1e-3, 1.0, 1.0, 64), ((1,), 1e-2, 4.0, 0.25, 64),
         ((3,), 1e-3, 1.0, 1.0, 64)]


@pytest.mark.parametrize("d", [1, 2, 17, 32])
def test_four_plans_and_one_that_fails_equal_the_definition_in_every_bit(d):
    """T = 1, 2 and 64; group 3 is empty, so the fifth plan has too few samples; M, K, delta and status as bytes"""
    a, y, groups, lo, span, rest = filter_case(240, d, seed=20 + d)
    c = KF.centre(lo, span, rest)
    mom = KF.moments(torch.from_numpy(a).cuda(), y, groups, 4, c)
    ref_mom = KF.moments_reference(a, y, groups, 4, c)
    assert all(same_bits(mom[k].cpu().numpy(), ref_mom[k]) for k in ("G", "C", "S", "E"))
    want = KF.design_reference(ref_mom, PLANS)
    assert want["status"].tolist() == [0, 0, 0, 0, 1] and want["M"][:4].any(axis=(1, 2)).all() and not want["M"][4].any()
    print(f"D = {d}: delta", want["delta"].tolist())
    for order in (PLANS, [PLANS[4]] + PLANS[:4]):
        sel = [PLANS.index(p) for p in order]
        got = {k: v.cpu().numpy() for k, v in KF.design(mom, order).items()}
        assert same_bits(got["status"], want["status"][sel])
        for key in ("M", "K", "delta"):
            assert same_bits(got[key], want[key][sel]), (key, d, got[key][0].ravel()[:4], want[key][sel][0].ravel()[:4])


def test_a_matrix_that_is_not_positive_definite_ends_the_plan():
    a, y, _, lo, span, rest = filter_case(40, 2, seed=3)
    c = KF.centre(lo, span, rest)
    a, y = np.tile(a[:1], (40, 1)), np.tile(y[:1], (40, 1))    # the hand does not move: omega = 0 and G is singular
    plans = [(1, 0.0, 1.0, 1.0, 4), (1, 1e-3, 1.0, 1.0, 4)]
    want = KF.design_reference(KF.moments_reference(a, y, None, 1, c), plans)
    got = {k: v.cpu().numpy() for k, v in KF.design(KF.moments(torch.from_numpy(a).cuda(), y, None, 1, c), plans).items()}
    assert want["status"][0] == 2 and all(same_bits(got[k], want[k]) for k in ("M", "K", "delta", "status")), (got["status"], want["status"])


@pytest.fixture(scope="module")
def rows100():
    """100 rows of tail inputs, a readout of 20 joints and a filter fitted to its output against a smoothed copy of it"""
    rng = np.random.default_rng(30)
    u = np.maximum(rng.standard_normal((100, 512)) + 0.2, 0.0).astype(F)
    W, b, lo, span, rest = model(20, 31, u)
    a = K.pose_reference(u, W, b)
    y = np.stack([a[max(i - 2, 0):i + 3].mean(axis=0) for i in range(100)]).astype(F)
    c = KF.centre(lo, span, rest)
    des = KF.design_reference(KF.moments_reference(a, y, None, 1, c), [(1, 1e-3, 1.0, 1.0, 32), (1, 1e-3, 1.0, 8.0, 32)])
    assert des["status"].tolist() == [0, 0]
    return u, (W, b, lo, span, rest), a, y, c, des


def test_the_sweep_equals_the_definition_and_a_freshly_reset_stage(rows100):
    """two plans x 100 rows: the eight sums and the filtered rows as bytes; the filtered rows of a plan whose mask holds every
    row are those of a stage with that plan on the same rows"""
    u, mod, a, y, c, des = rows100
    groups = np.zeros(100, dtype=np.int64)
    groups[60:] = 1
    groups[30] = -1
    u_dev = torch.from_numpy(u).cuda()
    a_dev = K.apply(u_dev, mod[0], mod[1])[0]
    assert same_bits(a_dev.cpu().numpy(), a)
    for masks in ([0b01, 0b10], [0b11, 0b00]):
        want_s, want_f = KF.sweep_reference(a, y, groups, masks, des["M"], des["K"], c, return_filtered=True)
        sums, filt = KF.sweep(a_dev, y, groups, masks, des["M"], des["K"], c, return_filtered=True)
        assert same_bits(sums.cpu().numpy(), want_s), np.abs(sums.cpu().numpy() - want_s).max()
        assert same_f32(filt.cpu().numpy(), want_f)
        assert same_bits(KF.sweep(a_dev, y, groups, masks, des["M"], des["K"], c).cpu().numpy(), want_s)
    one = np.zeros(100, dtype=np.int64)
    filt = KF.sweep(a_dev, y, one, [1, 1], des["M"], des["K"], c, return_filtered=True)[1]
    for p in range(2):
        stage = KF.PoseFilter(Source())
        stage.set_model(*mod, des["M"][p], des["K"][p])
        stage.reset()
        got = stage.apply(u_dev)
        assert torch.equal(got[1], filt[p]) and torch.equal(got[0], a_dev), p


# ---------------------------------------------------------------------------------------------------------------------------
# the stage against FilterReference
# ---------------------------------------------------------------------------------------------------------------------------
def run_cuts(stage, u_dev, cls_dev, cut):
    n = int(u_dev.shape[0])
    step = n if cut is None else cut
    parts = [stage.apply(u_dev[s:s + step], None if cls_dev is None else cls_dev[s:s + step]) for s in range(0, n, step)]
    return [torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(4)]


@pytest.mark.parametrize("with_cls", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_stage_equals_the_definition_for_any_cut(rows100, dtype, with_cls):
    u, mod, _, _, _, des = rows100
    rng = np.random.default_rng(40)
    u = u.copy()
    u[0], u[47] = np.nan, np.nan                               # a row before the start and a held row
    u, u_dev = stored(u, dtype)
    cls = np.where(rng.random(100) < 0.2, -1, 3).astype(np.int32) if with_cls else None
    cls_dev = None if cls is None else torch.from_numpy(cls).cuda()
    ref = KF.FilterReference(des["M"][0], des["K"][0], *mod[2:], rate=300)
    raw = K.pose_reference(u, mod[0], mod[1])
    want = (raw,) + ref.push(raw, cls)
    assert EVENTS - {"none"} <= ref.events and ("none" in ref.events) == with_cls
    first_ws = None
    for cut in CUTS:
        stage = KF.PoseFilter(Source(dtype=dtype), rate=300)
        stage.set_model(*mod, des["M"][0], des["K"][0])
        got = run_cuts(stage, u_dev, cls_dev, cut)
        for name, g, w in zip(NAMES, got, want):
            assert same(g, w), (cut, name)
        st = stage.state()
        assert st["joints"] == 20 and st["started"] and same_bits(st["x"], ref.state()["x"]) and same_bits(st["out"], ref.state()["out"])
        ws = stage.ws.cpu().numpy()
        first_ws = ws if first_ws is None else first_ws
        assert same_bits(ws, first_ws), cut                    # the whole workspace, whatever the cut
    stage.reset()
    assert not stage.state()["out"].any() and not stage.state()["started"] and not stage.state()["x"].any()
    assert all(same(g, w) for g, w in zip(run_cuts(stage, u_dev, cls_dev, 17), want))
    joint = K.JointAngles(Source(dtype=dtype), smooth=1)
    joint.set_model(*mod)
    assert torch.equal(joint.apply(u_dev)[0].view(torch.int32), stage_raw(stage, u_dev).view(torch.int32))      # raw is JointAngles' raw


def stage_raw(stage, u_dev):
    stage.reset()
    return stage.apply(u_dev)[0]


def test_the_stage_reaches_every_event_of_the_definition():
    """the crafted rows of the host test through a readout that selects its inputs (a = u exactly)"""
    M, Kg, lo, span, rest, a, cls = crafted_rows()
    W = np.zeros((2, 512), dtype=F)
    W[0, 0], W[1, 1] = 1.0, 1.0
    u = np.zeros((32, 512), dtype=F)
    u[:, :2] = a
    raw = K.pose_reference(u, W, np.zeros(2, dtype=F))         # (a where a is finite; a non-finite input reaches both joints)
    assert same_bits(raw[2:6], a[2:6]) and not np.isfinite(raw[[0, 1, 6, 7]]).any()
    ref = KF.FilterReference(M, Kg, lo, span, rest, rate=600)
    want = (raw,) + ref.push(raw, cls)
    assert ref.events == EVENTS
    u_dev, cls_dev = torch.from_numpy(u).cuda(), torch.from_numpy(cls.astype(np.int32)).cuda()
    for cut in (1, 16, None):
        stage = KF.PoseFilter(Source(), rate=600)
        stage.set_model(W, np.zeros(2, dtype=F), lo, span, rest, M, Kg)
        got = run_cuts(stage, u_dev, cls_dev, cut)
        assert all(same(g, w) for g, w in zip(got, want)), cut


def test_streams_that_share_a_launch_equal_their_own_stages(rows100):
    """four streams in one launch of the C entry: one with rows, one with a model and m = 0, one with rows and no model, one
    with another model, 17 joints and a class input; each against a single-stream stage of its own"""
    u, mod, a, y, c, des = rows100
    rng = np.random.default_rng(50)
    u_dev = torch.from_numpy(u[:70]).cuda()
    ma = mod + (des["M"][0], des["K"][0])
    keep = np.r_[0:17, 20:37]
    mb = tuple(v[:17] for v in mod) + (np.ascontiguousarray(des["M"][1][np.ix_(keep, keep)]), np.ascontiguousarray(des["K"][1][keep, :17]))
    cls = torch.from_numpy(np.where(rng.random(70) < 0.3, -1, 1).astype(np.int32)).cuda()
    multi = KF.PoseFilter(Source(4), rate=500)
    multi.set_model(0, *ma)
    multi.set_model(1, *mb)
    multi.set_model(3, *mb)
    row0, m = np.array([0, 30, 30, 45]), np.array([30, 0, 15, 25])
    singles = []
    for s, mod_s in ((0, ma), (1, mb), (3, mb)):
        one = KF.PoseFilter(Source(), rate=500)
        one.set_model(*mod_s)
        singles.append((s, one))
    for half in (0, 1):                                        # two launches: the state carries over
        lo_rows = [int(r0 + half * (n // 2)) for r0, n in zip(row0, m)]
        n_rows = [int(n // 2 if half == 0 else n - n // 2) for n in m]
        r0 = np.zeros(4, dtype=np.int64)
        np.cumsum(np.array(n_rows)[:-1], out=r0[1:])
        tail = torch.cat([u_dev[s:s + n] for s, n in zip(lo_rows, n_rows)])
        cl = torch.cat([cls[s:s + n] for s, n in zip(lo_rows, n_rows)])
        rows = int(sum(n_rows))
        rm = torch.from_numpy(np.stack([r0, np.array(n_rows)]).astype(np.int32)).cuda()
        outs = [torch.full((rows, 32), -7.0, device="cuda"), torch.full((rows, 32), -7.0, device="cuda"),
                torch.full((rows, 32), -7, dtype=torch.int32, device="cuda"), torch.full((rows, 32), -7.0, device="cuda")]
        _lib.check(multi.lib.cp_online_kf_push(*multi._args(), tail.data_ptr(), _lib.CP_F32, 512, cl.data_ptr(), rm[0].data_ptr(),
                                               rm[1].data_ptr(), rows, *(o.data_ptr() for o in outs), multi._stream()),
                   "cp_online_kf_push")
        for s, one in singles:
            at, n = int(r0[s]), n_rows[s]
            if n == 0:
                continue
            want = one.apply(tail[at:at + n], cl[at:at + n])
            d = one._joints[0]
            for got, w in zip(outs, want):
                assert torch.equal(got[at:at + n, :d], w) and not got[at:at + n, d:].any(), (half, s)
        at, n = int(r0[2]), n_rows[2]                          # the stream without a model: its rows keep their sentinel
        assert all((o[at:at + n] == -7).all() for o in outs)
    per = 4 * KF._STATE_WORDS
    ws = multi.ws.cpu().numpy()
    for s, one in singles:
        assert same_bits(ws[s * per:(s + 1) * per], one.ws.cpu().numpy()[:per]), s
    assert not ws[2 * per:3 * per].any()
    assert not multi.state(1)["started"] and multi.state(3)["started"] and multi.state(2)["joints"] == 0
    with pytest.raises(_lib.CpNativeError, match="no pose model"):
        multi.apply([None, None, u_dev[:3], None])
    got = multi.apply([u_dev[:10], None, None, u_dev[10:30]], [cls[:10], None, None, cls[10:30]])
    assert got[1][0].shape == (0, 17) and got[0][1].shape == (10, 20) and got[3][2].shape == (20, 17) and len(got[0]) == 4


# ---------------------------------------------------------------------------------------------------------------------------
# behind the decoders
# ---------------------------------------------------------------------------------------------------------------------------
def probe_filter(tail, d, seed):
    """a readout of d joints on the tail inputs a decoder left, and a filter fitted to its output"""
    W, b, lo, span, rest = model(d, seed, tail)
    a = K.pose_reference(tail, W, b)
    y = np.stack([a[max(i - 2, 0):i + 3].mean(axis=0) for i in range(a.shape[0])]).astype(F)
    des = KF.design_reference(KF.moments_reference(a, y, None, 1, KF.centre(lo, span, rest)), [(1, 1e-2, 1.0, 2.0, 24)])
    assert des["status"].tolist() == [0]
    return (W, b, lo, span, rest, des["M"][0], des["K"][0])


def check_rows(posed, tail, cls, ref, W, b):
    """raw, filtered, pose, angle of some rows against the definitions on the tail inputs read back"""
    raw = K.pose_reference(host(tail), W, b)
    want = (raw,) + ref.push(raw, None if cls is None else cls.cpu().numpy())
    for name, g, w in zip(NAMES, posed, want):
        assert same(g.cpu().numpy(), w), name


@pytest.mark.parametrize("dtype,adapt", [("f32", None), ("bf16", None), ("f32", 0.02), ("bf16", 0.02)])
def test_behind_a_push_the_source_is_unchanged_and_the_pose_is_the_definitions(engine, recording, dtype, adapt):
    """`PoseFilter(OnlineDecoder)` and `PoseFilter(CommandGate(...))`, folded and adaptive.  Three decoders take the same chunks
    of 1, 16, 17, 25 and 40 windows (the last more than the decoder runs in one chain of launches): one under the stage, a twin
    under a `JointAngles` (the source's own outputs and `raw`), and one under a second stage that is fed pieces of at most one
    chain, so that `tail_view()` holds every row it has just posed: those rows are held to the definitions on the values read
    back, and the first stage's rows to theirs."""
    raw, labels, norm, _ = recording
    make = lambda: OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, vote=9, max_windows_per_push=32, adapt=adapt)
    probe = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, vote=9, adapt=adapt)
    probe.push(raw[:2000])
    mod = probe_filter(host(probe.tail_view()[:96]), 20, 51)   # (20 joints need 41 samples)
    for gated in (False, True):
        decs = [make(), make(), make()]
        srcs = [CommandGate(d, min_cosine=0.2, dwell=2) for d in decs] if gated else decs
        stage, pieces = KF.PoseFilter(srcs[0], rate=400), KF.PoseFilter(srcs[2], rate=400)
        twin = K.JointAngles(srcs[1], smooth=1)
        stage.set_model(*mod)
        pieces.set_model(*mod)
        twin.set_model(*mod[:5])
        ref = KF.FilterReference(mod[5], mod[6], *mod[2:5], rate=400)
        at = 0
        for windows in (1, 16, 17, 25, 40):
            chunk = raw[at:at + 20 * windows]
            at += 20 * windows
            got = stage.push(chunk, return_logits=True)
            want = twin.push(chunk, return_logits=True)
            assert len(got) == len(want) + 1
            for i, (g, w) in enumerate(zip(got[:-4], want[:-3])):  # the source's own outputs, bit for bit
                assert torch.equal(g, w), (gated, windows, i)
            assert torch.equal(got[-4].view(torch.int32), want[-3].view(torch.int32)), (gated, windows, "raw")
            m = int(got[0].shape[0])
            assert tuple(got[-1].shape) == (m, 20) and got[-2].dtype == torch.int32 and got[-3].dtype == torch.float32
            parts = []
            for lo_s in range(0, chunk.shape[0], 20 * 32):     # one chain each: the view holds the rows just posed
                part = pieces.push(chunk[lo_s:lo_s + 20 * 32])
                mp = int(part[0].shape[0])
                check_rows(part[-4:], decs[2].tail_view()[:mp], part[-8] if gated else None, ref, mod[0], mod[1])   # [-8]: the gate's command
                parts.append(part[-4:])
            for i in range(4):
                assert torch.equal(got[-4 + i], torch.cat([p[i] for p in parts])), (gated, windows, i)
        assert same_bits(stage.ws.cpu().numpy(), pieces.ws.cpu().numpy())
        decs[0].push(raw[:40])
        with pytest.raises(_lib.CpNativeError, match="behind the stage"):
            stage.push(raw[40:80])
        stage.reset()
        assert int(decs[0].n_seen) == 0 and not stage.state()["out"].any() and not stage.state()["started"]
        assert stage.push(raw[:400])[-1].shape == (20, 20)
    with pytest.raises(_lib.CpNativeError, match="no pose model"):
        KF.PoseFilter(make()).push(raw[:400])


def test_a_stream_of_a_multi_stream_decoder_filters_as_its_own_decoder(engine, recording):
    """`PoseFilter(MultiStreamDecoder)` and `PoseFilter(AdaptiveMultiStreamDecoder)`: stream s against `PoseFilter` over an
    `OnlineDecoder` fed the same chunks; one push is larger than the decoder runs in one chain"""
    raw, labels, norm, _ = recording
    probe = OnlineDecoder(engine, *norm, classes=IDS, dtype="f32")
    probe.push(raw[:2000])
    tail = host(probe.tail_view()[:64])
    ma, mb = probe_filter(tail, 17, 61), probe_filter(tail, 5, 62)
    for adaptive in (False, True):
        if adaptive:
            multi = AdaptiveMultiStreamDecoder(engine, *norm, 3, 0.02, vote=9, dtype="f32", max_windows_per_push=16)
        else:
            multi = MultiStreamDecoder(engine, *norm, 3, vote=9, dtype="f32", max_windows_per_push=16)
        singles = [OnlineDecoder(engine, *norm, classes=IDS, dtype="f32", vote=9, max_windows_per_push=16, adapt=0.02 if adaptive else None)
                   for _ in range(3)]
        for s in range(3):
            multi.set_classes(s, classes=IDS)
        stage = KF.PoseFilter(multi, rate=700)
        stage.set_model(0, *ma)
        stage.set_model(2, *mb)
        ones = [KF.PoseFilter(singles[0], rate=700), None, KF.PoseFilter(singles[2], rate=700)]
        ones[0].set_model(*ma)
        ones[2].set_model(*mb)
        at = [0, 0, 3000]
        for sizes in ((140, 0, 333), (20, 0, 0), (500, 0, 25), (0, 0, 321)):
            chunks = [None if n == 0 else raw[s:s + n] for s, n in zip(at, sizes)]
            at = [s + n for s, n in zip(at, sizes)]
            got = stage.push(chunks)
            for s in (0, 2):
                want = ones[s].push(raw[at[s] - sizes[s]:at[s]])
                assert len(got[s]) == len(want) == 6
                for i, (g, w) in enumerate(zip(got[s], want)):
                    assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (adaptive, sizes, s, i)
            assert got[1][0].shape[0] == 0
        packed = stage.push_packed(torch.cat([raw[at[0]:at[0] + 100], raw[at[2]:at[2] + 60]]), [100, 0, 60])
        for s, n in ((0, 100), (2, 60)):
            want = ones[s].push(raw[at[s]:at[s] + n])
            assert all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(packed[s], want))
        with pytest.raises(_lib.CpNativeError, match="no pose model"):
            stage.push([None, raw[:100], None])
        stage.reset([0])
        assert not stage.state(0)["started"] and stage.state(2)["started"] and multi.n_seen[0] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the cross-fit, the fit and the pick
# ---------------------------------------------------------------------------------------------------------------------------
def pose_fit(u_dev, y, rep, cls, lag):
    """the readout on every repetition at ridge 0.01, as `fit_pose` fits it, from tail inputs"""
    groups, n_rep = rep
    G, Cm = K.moments(u_dev, y, None, groups, n_rep)
    W, b, st = K.solve(G, Cm, [(tuple(range(n_rep)), 0.01)], int(y.shape[1]))
    lo, span, rest = K.limits(y, cls, 0)
    return K.PoseFit(W, b, st.cpu().numpy(), [(tuple(range(n_rep)), 0.01)], {}, lo, span, rest, lag)


def test_crossfit_equals_the_definition_on_the_small_synthetic_person():
    p = K.kinematics_recording(k=4, reps=3, segment=12, joints=3, delay=2, seed=0)
    y = K.window_targets(p["glove"], 0, 2)
    n = int(y.shape[0])
    rep = (p["rep"][:n].copy(), p["n_rep"])
    rep[0][5] = -1                                             # a window without a repetition: NaN
    got = KF.crossfit_inputs(torch.from_numpy(p["u"][:n]).cuda(), y, rep, 0.01).cpu().numpy()
    want = KF.crossfit_reference(p["u"][:n], y, rep, 0.01)
    assert np.isnan(want[5]).all() and same_f32(got, want)


@pytest.mark.parametrize("lag", [0, 2])
def test_pick_filter_on_the_synthetic_person_equals_the_definitions_and_helps(lag):
    """`kinematics_recording(6, 3, 30, 20)` behind the encoder (its synthetic tail inputs): the cross-fitted readout, then every
    table of `pick_filter` against `pick_filter_reference` on the same a; the pick is a filtered row below the unfiltered one"""
    p = K.kinematics_recording(6, 3, 30, 20)
    y = K.window_targets(p["glove"], 0, lag)
    n = int(y.shape[0])
    rep = (p["rep"][:n], p["n_rep"])
    u_dev = torch.from_numpy(p["u"][:n]).cuda()
    a = KF.crossfit_inputs(u_dev, y, rep, 0.01)
    fit = pose_fit(u_dev, y, rep, p["cls"][:n], lag)
    out = KF.pick_filter(a, y, rep, fit, iters=64)
    ref = KF.pick_filter_reference(a.cpu().numpy(), y, rep, fit, iters=64)
    print(f"lag {lag}: rho, kappa, mean held-out RMSE, jitter\n", out["table"], "\npick", out["pick"], "delta", out["delta"].max())
    assert out["table"].shape == (4, 4) and out["sums"].shape == (4, 20, 8) and out["ok"].all()
    for key in ("table", "sums", "fold_sums", "bare_fold_sums", "ok", "delta", "rmse", "rmse_mean", "jitter"):
        assert same_bits(out[key], ref[key]) or (key == "table" and same_bits(out[key][:, 2:], ref[key][:, 2:])), key
    assert out["pick"] == ref["pick"] and out["pick"] >= 1 and out["kappa"] == ref["kappa"]
    assert out["table"][out["pick"], 2] < out["table"][0, 2]
    # the picked filter, fitted on every repetition and installed, filters a stream of the person's tail inputs
    model_fit = KF.fit_filter(a, y, rep, fit, kappa=out["kappa"], rho=out["rho"], iters=64)
    want = KF.design_reference(KF.moments_reference(a.cpu().numpy(), y, rep[0], 3, model_fit.centre), [(7, 1e-3, out["rho"], out["kappa"], 64)])
    assert model_fit.status.tolist() == [0] and same_bits(model_fit.M.cpu().numpy(), want["M"]) and same_bits(model_fit.delta, want["delta"])
    assert sum(model_fit.counts.values()) == n - 2 * 3 and same_bits(model_fit.centre, KF.centre(fit.lo, fit.span, fit.rest))
    stage = KF.PoseFilter(Source(), fit, model_fit)
    got = stage.apply(u_dev[:50])
    ref_stage = KF.FilterReference(want["M"][0], want["K"][0], fit.lo, fit.span, fit.rest)
    raw = K.pose_reference(p["u"][:50], fit.W[0].cpu().numpy(), fit.b[0].cpu().numpy())
    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, (raw,) + ref_stage.push(raw)))


def test_crossfit_behind_a_decoder_equals_the_definition_and_leaves_it_alone(engine, recording):
    raw, labels, norm, glove = recording
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype="f32", vote=9)
    dec.push(raw[:777])                                        # a stream in mid-flight with a filled vote ring
    expected = window_labels(labels)
    m = int(expected.shape[0])
    rep, n_rep = H.repetitions(expected)
    before = dec.ws.clone(), dec.n_seen, [t.clone() for t in dec.projection()], [t.clone() for t in dec.class_table()]
    a = KF.crossfit_pose(dec, raw, glove, (rep, n_rep), ridge=1.0, lag=2)
    fit = K.fit_pose(dec, raw, glove, rep=(rep, n_rep), ridge=[1.0], lag=2, labels=labels, rest_label=IDS[0])
    y = K.window_targets(glove, 0, 2)
    n = int(y.shape[0])
    model_fit = KF.fit_filter(a, y, (rep[:n], n_rep), fit, iters=16)
    u = dec._recording_tail_inputs(None, raw, np.arange(n))
    after = dec.ws.clone(), dec.n_seen, dec.projection(), dec.class_table()
    n_state = H._state_bytes(dec, False)
    assert torch.equal(before[0][:n_state], after[0][:n_state]) and before[1] == after[1] == 777
    assert all(torch.equal(x, z) for x, z in zip(before[2], after[2])) and all(torch.equal(x, z) for x, z in zip(before[3], after[3]))
    want = KF.crossfit_reference(host(u), y, (rep[:n], n_rep), 1.0)
    assert a.shape == (n, 5) and same_f32(a.cpu().numpy(), want)
    c = KF.centre(fit.lo, fit.span, fit.rest)
    des = KF.design_reference(KF.moments_reference(want, y, rep[:n], n_rep, c), [((1 << n_rep) - 1, 1e-3, 1.0, 1.0, 16)])
    assert same_bits(model_fit.M.cpu().numpy(), des["M"]) and same_bits(model_fit.K.cpu().numpy(), des["K"])
    assert same_bits(model_fit.status, des["status"]) and same_bits(model_fit.delta, des["delta"])
    # installed through the constructor, the stage's raw output is the readout's apply
    stage = KF.PoseFilter(dec, fit, model_fit)
    stage.reset()
    got = stage.push(raw[:20 * 30 + 10])
    assert got[2].shape == got[3].shape == got[4].shape == got[5].shape == (30, 5)
    assert torch.equal(got[2], fit.apply(dec, raw)[0][:30])
