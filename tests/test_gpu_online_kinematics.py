"""Joint-angle decoding on the MI355X (contrastiveprosthetics_amd/kinematics.py, csrc/online_kinematics.cuh) against the numpy
definitions, in every bit: the moments, the fit through cp_online_readout_solve, the apply and the score, the stage against
`JointReference` for any cut of the rows and any set of streams in a launch, `tail_view()` against cp_online_*tail_inputs, the
stage behind a push of every decoder form and of a gate, and `pick_pose`'s tables."""
import numpy as np
import pytest
import torch

from contrastiveprosthetics_amd import _lib
from contrastiveprosthetics_amd import holdout as H
from contrastiveprosthetics_amd import kinematics as K
from contrastiveprosthetics_amd import readout as R
from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, CommandGate, MultiStreamDecoder, OnlineDecoder, window_labels
from test_gpu_online_readout import IDS, cued
from test_gpu_online_track import _engine
from test_online_kinematics_host import EVENTS, crafted_rows, same_bits, small_case

pytestmark = pytest.mark.gpu

F = np.float32
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
CUTS = [1, 16, 17, 25, None]                                   # rows per call; None: all at once


@pytest.fixture(scope="module")
def engine():
    return _engine()


def stored(u, dtype):
    """u as a decoder of `dtype` stores it: (numpy f32 values, the tensor on the GPU)"""
    v = u if dtype == "f32" else R.round_bf16(u).astype(F)
    return v, torch.from_numpy(v).cuda().to(TORCH[dtype])


def host(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


class Source:
    """what `JointAngles` asks of a decoder, for the tests that drive the stage alone (`apply`)"""

    def __init__(self, n_streams=None, dtype="f32"):
        self.class_ids = None if n_streams is None else [None] * n_streams
        self.n_seen = 0 if n_streams is None else np.zeros(n_streams, dtype=np.int64)
        self.device, self.dtype = torch.device("cuda:0"), dtype

    def push(self, *a, **k):
        raise AssertionError("not pushed")

    tail_view = push

    def reset(self, streams=None):
        pass


def same_f32(got, want):
    """f32 arrays as bit patterns; where both hold a NaN its payload is not compared (the definition does not fix one)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != F or want.dtype != F:
        return False
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


# ---------------------------------------------------------------------------------------------------------------------------
# moments, fit, apply and score against the definitions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, R.STAGE - 1, R.STAGE, R.STAGE + 1, 100])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_moments_equal_the_definition_in_every_bit(dtype, n):
    """three groups of which group 1 is empty, unused windows (group -1) among the rest; D = 1, 16, 17, 20 and 32 joints.  A
    joint's column of C does not depend on the other joints, so one definition at 32 joints serves every D."""
    u, y, groups = small_case(n, 32, seed=10 + n, n_groups=3)
    groups[groups == 1] = 2
    if n >= R.STAGE - 1:
        assert (groups < 0).any() and (groups >= 0).any()
    u, u_dev = stored(u, dtype)
    want_g, want_c = K.moments_reference(u, y, None, groups, 3)
    assert not want_g[1].any() and not want_c[1].any()
    for d in (1, 16, 17, 20, 32):
        G, Cm = K.moments(u_dev, np.ascontiguousarray(y[:, :d]), None, groups, 3)
        got_g, got_c = G.cpu().numpy(), Cm.cpu().numpy()
        assert same_bits(got_g, want_g), ("G", d, np.abs(got_g - want_g).max())
        blocks = K.column_blocks(want_c[:, :, :d])
        assert got_c.shape == (2, 3, 513, 16) and same_bits(got_c, blocks), ("C", d, np.abs(got_c - blocks).max())


def test_an_empty_recording_gives_zero_moments():
    G, Cm = K.moments(torch.empty(0, 512, device="cuda"), np.zeros((0, 3), F), None, None, 2)
    assert not G.cpu().numpy().any() and not Cm.cpu().numpy().any()


@pytest.fixture(scope="module")
def fit100():
    """100 windows < 513 unknowns, 20 joints (two column blocks), group 1 empty; four plans and a fifth that fails"""
    u, y, groups = small_case(100, 20, seed=1, n_groups=3)
    groups[groups == 1] = 2
    plans = [((0, 2), 1e-4), ((0, 2), 1.0), ((0,), 1e-4), ((0,), 1.0), ((1,), 0.0)]
    want = K.fit_reference(u, y, plans, groups=groups, n_groups=3)
    assert want["status"].tolist() == [0, 0, 0, 0, 1] and not want["W"][4].any() and not want["b"][4].any()
    return u, y, groups, plans, want


def test_four_plans_and_one_that_fails(fit100):
    u, y, groups, plans, want = fit100
    G, Cm = K.moments(torch.from_numpy(u).cuda(), y, None, groups, 3)
    assert same_bits(G.cpu().numpy(), want["G"]) and same_bits(Cm.cpu().numpy(), K.column_blocks(want["C"]))
    for order, sel in ((plans, [0, 1, 2, 3, 4]), ([plans[4]] + plans[:4], [4, 0, 1, 2, 3])):
        W, b, status = (x.cpu().numpy() for x in K.solve(G, Cm, order, 20))
        assert W.shape == (5, 20, 512) and b.shape == (5, 20)
        assert same_bits(status, want["status"][sel])
        assert same_bits(W, want["W"][sel]), np.abs(W - want["W"][sel]).max()
        assert same_bits(b, want["b"][sel]), np.abs(b - want["b"][sel]).max()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_apply_and_score_equal_the_definitions_in_every_bit(fit100, dtype):
    """two plans x 100 rows x 20 joints; the score of plan 0 on group 0, of plan 1 on groups 0 and 2"""
    u, y, groups, plans, want = fit100
    u, u_dev = stored(u, dtype)
    W, b = want["W"][:2], want["b"][:2]
    pred = K.apply(u_dev, W, b)
    ref = np.stack([K.pose_reference(u, W[p], b[p]) for p in range(2)])
    got = pred.cpu().numpy()
    assert got.shape == (2, 100, 20) and same_bits(got, ref), np.abs(got - ref).max()
    assert same_bits(K.apply(u_dev, W[1], b[1]).cpu().numpy(), ref[1:2])
    sums = K.score(pred, y, groups, [0b001, 0b101]).cpu().numpy()
    want_sums = K.score_reference(ref, y, groups, [0b001, 0b101])
    assert sums.shape == (2, 20, 7) and sums[0, 0, 0] == (groups == 0).sum() and sums[1, 0, 0] == (groups >= 0).sum()
    assert same_bits(sums, want_sums), np.abs(sums - want_sums).max()
    assert K.apply(u_dev[:0], W, b).shape == (2, 0, 20) and not K.score(pred[:, :0], y[:0], groups[:0], [1, 1]).cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------------------
# the stage against JointReference
# ---------------------------------------------------------------------------------------------------------------------------
def model(d, seed, u):
    """a readout of d joints whose levels cross both bounds on the rows u"""
    rng = np.random.default_rng(seed)
    W = (0.05 * rng.standard_normal((d, 512))).astype(F)
    b = rng.standard_normal(d).astype(F)
    a = K.pose_reference(u, W, b)
    lo, span, rest = K.limits(a, low=10.0, high=90.0)          # a fifth of the rows clamps
    return W, b, lo, span, rest


def run_cuts(stage, u_dev, cls_dev, cut):
    n = int(u_dev.shape[0])
    step = n if cut is None else cut
    parts = [stage.apply(u_dev[s:s + step], None if cls_dev is None else cls_dev[s:s + step]) for s in range(0, n, step)]
    return [torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(3)]


@pytest.mark.parametrize("with_cls", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_stage_equals_the_definition_for_any_cut(dtype, with_cls):
    rng = np.random.default_rng(20)
    u, u_dev = stored(np.maximum(rng.standard_normal((100, 512)) + 0.2, 0.0).astype(F), dtype)
    W, b, lo, span, rest = model(20, 21, u)
    cls = np.where(rng.random(100) < 0.2, -1, 3).astype(np.int32) if with_cls else None
    cls_dev = None if cls is None else torch.from_numpy(cls).cuda()
    ref = K.JointReference(W, b, lo, span, rest, smooth=5, rate=300)
    want = ref.push(u, cls)
    assert {"clamp_low", "clamp_high", "ring_filling", "rise_limited", "fall_limited"} <= ref.events and ("none" in ref.events) == with_cls
    first_ws = None
    for cut in CUTS:
        stage = K.JointAngles(Source(dtype=dtype), smooth=5, rate=300)
        stage.set_model(W, b, lo, span, rest)
        got = run_cuts(stage, u_dev, cls_dev, cut)
        for name, g, w in zip(("raw", "pose", "angle"), got, want):
            assert same_bits(g, w), (cut, name)
        st = stage.state()
        assert st["joints"] == 20 and same_bits(st["out"], ref.state()["out"]) and same_bits(st["ring"], ref.state()["ring"])
        ws = stage.ws.cpu().numpy()
        first_ws = ws if first_ws is None else first_ws
        assert same_bits(ws, first_ws), cut                    # the whole workspace, whatever the cut
    stage.reset()
    assert not stage.state()["out"].any() and stage.state()["ring"].shape == (0, 20)
    assert all(same_bits(g, w) for g, w in zip(run_cuts(stage, u_dev, cls_dev, 17), want))


def test_the_stage_reaches_every_event_of_the_definition():
    """the crafted rows of the host test: clamps, a NaN row, the class "none", rate-limited rise and fall, a ring not yet full"""
    W, b, lo, span, rest, u, cls = crafted_rows()
    ref = K.JointReference(W, b, lo, span, rest, smooth=4, rate=600)
    want = ref.push(u, cls)
    assert ref.events == EVENTS
    u_dev, cls_dev = torch.from_numpy(u).cuda(), torch.from_numpy(cls.astype(np.int32)).cuda()
    for cut in (1, 16, None):
        stage = K.JointAngles(Source(), smooth=4, rate=600)
        stage.set_model(W, b, lo, span, rest)
        got = run_cuts(stage, u_dev, cls_dev, cut)
        assert np.isnan(want[0]).any() and not np.isnan(want[2]).any()
        assert same_bits(got[1], want[1]) and same_f32(got[0], want[0]) and same_bits(got[2], want[2])
    plain = K.JointAngles(Source(), smooth=1, rate=K.ONE)      # no smoothing, no rate limit, no class input: pose = q
    plain.set_model(W, b, lo, span, rest)
    ref1 = K.JointReference(W, b, lo, span, rest, smooth=1, rate=K.ONE)
    ref1.push(u)
    assert same_bits(plain.apply(u_dev)[1].cpu().numpy().astype(np.int64), ref1.q)


def test_streams_that_share_a_launch_equal_their_own_stages():
    """four streams in one launch of the C entry: one with rows, one with a model and m = 0, one with rows and no model, one
    with another model, 17 joints and a class input; each against a single-stream stage of its own"""
    rng = np.random.default_rng(30)
    u, u_dev = stored(np.maximum(rng.standard_normal((70, 512)) + 0.2, 0.0).astype(F), "f32")
    ma, mb = model(20, 31, u), model(17, 32, u)
    cls = torch.from_numpy(np.where(rng.random(70) < 0.3, -1, 1).astype(np.int32)).cuda()
    multi = K.JointAngles(Source(4), smooth=7, rate=500)
    multi.set_model(0, *ma)
    multi.set_model(1, *mb)
    multi.set_model(3, *mb)
    row0, m = np.array([0, 30, 30, 45]), np.array([30, 0, 15, 25])
    singles = []
    for s, mod in ((0, ma), (1, mb), (3, mb)):
        one = K.JointAngles(Source(), smooth=7, rate=500)
        one.set_model(*mod)
        singles.append((s, one))
    for half in (0, 1):                                        # two launches: the state carries over
        lo_rows = [int(r0 + half * (n // 2)) for r0, n in zip(row0, m)]
        n_rows = [int(n // 2 if half == 0 else n - n // 2) for n in m]
        r0 = np.zeros(4, dtype=np.int64)
        np.cumsum(np.array(n_rows)[:-1], out=r0[1:])
        tail = torch.cat([u_dev[a:a + n] for a, n in zip(lo_rows, n_rows)])
        c = torch.cat([cls[a:a + n] for a, n in zip(lo_rows, n_rows)])
        rows = int(sum(n_rows))
        rm = torch.from_numpy(np.stack([r0, np.array(n_rows)]).astype(np.int32)).cuda()
        raw = torch.full((rows, 32), -7.0, device="cuda")
        pose = torch.full((rows, 32), -7, dtype=torch.int32, device="cuda")
        angle = torch.full((rows, 32), -7.0, device="cuda")
        _lib.check(multi.lib.cp_online_kin_push(*multi._args(), tail.data_ptr(), _lib.CP_F32, 512, c.data_ptr(), rm[0].data_ptr(),
                                                rm[1].data_ptr(), rows, raw.data_ptr(), pose.data_ptr(), angle.data_ptr(),
                                                multi._stream()), "cp_online_kin_push")
        for s, one in singles:
            a, n = int(r0[s]), n_rows[s]
            if n == 0:
                continue
            want = one.apply(tail[a:a + n], c[a:a + n])
            d = one._joints[0]
            for got, w in zip((raw, pose, angle), want):
                assert torch.equal(got[a:a + n, :d], w) and not got[a:a + n, d:].any(), (half, s)
        a, n = int(r0[2]), n_rows[2]                           # the stream without a model: nothing of it is written
        assert (raw[a:a + n] == -7).all() and (pose[a:a + n] == -7).all() and (angle[a:a + n] == -7).all()
    per = 4 * K._STATE_WORDS
    ws = multi.ws.cpu().numpy()
    for s, one in singles:
        assert same_bits(ws[s * per:(s + 1) * per], one.ws.cpu().numpy()[:per]), s
    assert not ws[2 * per:3 * per].any()
    assert multi.state(1)["ring"].shape == (0, 17) and multi.state(3)["ring"].shape == (7, 17) and multi.state(2)["joints"] == 0
    with pytest.raises(_lib.CpNativeError, match="no pose model"):
        multi.apply([None, None, u_dev[:3], None])
    # through `apply`, streams of one width (the outputs are then split in one piece)
    same = K.JointAngles(Source(3), smooth=7, rate=500)
    for s in range(3):
        same.set_model(s, *mb)
    got = same.apply([u_dev[:10], None, u_dev[10:30]], [cls[:10], None, cls[10:30]])
    assert got[1][0].shape == (0, 17)
    for s, (a, n) in ((0, (0, 10)), (2, (10, 20))):
        one = K.JointAngles(Source(), smooth=7, rate=500)
        one.set_model(*mb)
        assert all(torch.equal(g, w) and g.shape == (n, 17) for g, w in zip(got[s], one.apply(u_dev[a:a + n], cls[a:a + n])))


# ---------------------------------------------------------------------------------------------------------------------------
# behind the decoders
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recording():
    raw, labels = cued()
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    w = preprocess_segments(raw[None], keep=20 * np.arange(256))[0]
    rng = np.random.default_rng(40)
    walk = np.cumsum(rng.standard_normal((raw.shape[0] // 20 + 2, 5)), axis=0)
    glove = np.ascontiguousarray(np.repeat(30.0 + 3.0 * walk, 20, axis=0)[:raw.shape[0]].astype(F))
    return raw, labels, (w.mean(0), w.std(0)), glove


def tail_inputs_of(dec, key, windows):
    """cp_online_*tail_inputs of normalised windows (n, 12), as `_recording_tail_inputs` calls it"""
    n = int(windows.shape[0])
    w = windows.contiguous()
    u = torch.empty(n, 512, dtype=TORCH[dec.dtype], device=dec.device)
    scratch = torch.empty(dec.lib.cp_online_enroll_scratch_bytes(n, dec._cfg.dtype), dtype=torch.uint8, device=dec.device)
    dec._tail_inputs_call(key, w.data_ptr(), n, u.data_ptr(), scratch.data_ptr(), scratch.numel())
    return u


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tail_view_holds_the_tail_inputs_of_the_last_push(engine, recording, dtype):
    """the folded single and multi-stream forms: after a push of 1, 16, 17 and 25 windows the view equals
    cp_online_*tail_inputs of the same windows in every byte"""
    raw, labels, norm, _ = recording
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, max_windows_per_push=32)
    view = dec.tail_view()
    assert tuple(view.shape) == (32, 512) and view.dtype == TORCH[dtype]
    assert view.untyped_storage().data_ptr() == dec.ws.untyped_storage().data_ptr()
    at = 0
    for windows in (1, 16, 17, 25):
        res = dec.push(raw[at:at + 20 * windows], return_windows=True)
        at += 20 * windows
        m = int(res[0].shape[0])
        assert m in (windows, windows - 1)
        got = dec.tail_view()[:m].clone()
        assert torch.equal(got.view(torch.uint8), tail_inputs_of(dec, None, res[2]).view(torch.uint8)), windows
    multi = MultiStreamDecoder(engine, *norm, 3, dtype=dtype, max_windows_per_push=32)
    for s in range(3):
        multi.set_classes(s, classes=IDS)
    assert tuple(multi.tail_view().shape) == (multi.max_rows, 512)
    at = 0
    for windows in (1, 16, 17, 25):
        chunks = [raw[at:at + 20 * windows], None, raw[5000 + at:5000 + at + 20 * windows + 20]]
        at += 20 * windows
        res = multi.push(chunks, return_windows=True)
        ws = torch.cat([r[2] for r in res])                    # packed (stream, window)
        got = multi.tail_view()[:ws.shape[0]].clone()
        assert ws.shape[0] >= 2 * windows - 1
        assert torch.equal(got.view(torch.uint8), tail_inputs_of(multi, 0, ws).view(torch.uint8)), windows


def check_rows(posed, tail, cls, ref):
    """raw, pose, angle of some rows against the definition on the tail inputs read back"""
    want = ref.push(host(tail), None if cls is None else cls.cpu().numpy())
    for name, g, w in zip(("raw", "pose", "angle"), posed, want):
        g = g.cpu().numpy()
        assert same_f32(g, w) if w.dtype == F else same_bits(g, w), name


@pytest.mark.parametrize("dtype,adapt", [("f32", None), ("bf16", None), ("f32", 0.02), ("bf16", 0.02)])
def test_behind_a_push_the_source_is_unchanged_and_the_pose_is_the_definitions(engine, recording, dtype, adapt):
    """`JointAngles(OnlineDecoder)` and `JointAngles(CommandGate(...))`, folded and adaptive.  Three decoders take the same
    chunks of 1, 16, 17, 25 and 40 windows (the last more than the decoder runs in one chain of launches): one under the stage,
    a twin without it (the source's own outputs), and one under a second stage that is fed pieces of at most one chain, so that
    `tail_view()` holds every row it has just posed: those rows are held to the definition on the values read back, and the
    first stage's rows to theirs."""
    raw, labels, norm, _ = recording
    make = lambda: OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, vote=9, max_windows_per_push=32, adapt=adapt)
    probe = make()
    probe.push(raw[:2000])
    W, b, lo, span, rest = model(20, 51, host(probe.tail_view()[:32]))
    for gated in (False, True):
        decs = [make(), make(), make()]
        srcs = [CommandGate(d, min_cosine=0.2, dwell=2) for d in decs] if gated else decs
        stage, pieces = K.JointAngles(srcs[0], smooth=5, rate=400), K.JointAngles(srcs[2], smooth=5, rate=400)
        stage.set_model(W, b, lo, span, rest)
        pieces.set_model(W, b, lo, span, rest)
        ref = K.JointReference(W, b, lo, span, rest, smooth=5, rate=400)
        at = 0
        for windows in (1, 16, 17, 25, 40):
            chunk = raw[at:at + 20 * windows]
            at += 20 * windows
            got = stage.push(chunk, return_logits=True)
            want = srcs[1].push(chunk, return_logits=True)
            assert len(got) == len(want) + 3
            for i, (g, w) in enumerate(zip(got, want)):        # the source's own outputs, bit for bit
                assert torch.equal(g, w), (gated, windows, i)
            m = int(got[0].shape[0])
            assert tuple(got[-1].shape) == (m, 20) and got[-2].dtype == torch.int32 and got[-3].dtype == torch.float32
            parts = []
            for lo_s in range(0, chunk.shape[0], 20 * 32):     # one chain each: the view holds the rows just posed
                part = pieces.push(chunk[lo_s:lo_s + 20 * 32])
                mp = int(part[0].shape[0])
                check_rows(part[-3:], decs[2].tail_view()[:mp], part[-7] if gated else None, ref)      # [-7]: the gate's command
                parts.append(part[-3:])
            for i in range(3):
                assert torch.equal(got[-3 + i], torch.cat([p[i] for p in parts])), (gated, windows, i)
        assert same_bits(stage.ws.cpu().numpy(), pieces.ws.cpu().numpy())
        decs[0].push(raw[:40])
        with pytest.raises(_lib.CpNativeError, match="behind the stage"):
            stage.push(raw[40:80])
        stage.reset()
        assert int(decs[0].n_seen) == 0 and not stage.state()["out"].any() and stage.state()["ring"].shape == (0, 20)
        assert stage.push(raw[:400])[-1].shape == (20, 20)
    with pytest.raises(_lib.CpNativeError, match="no pose model"):
        K.JointAngles(make()).push(raw[:400])


def test_a_stream_of_a_multi_stream_decoder_poses_as_its_own_decoder(engine, recording):
    """`JointAngles(MultiStreamDecoder)` and `JointAngles(AdaptiveMultiStreamDecoder)`: stream s against `JointAngles` over an
    `OnlineDecoder` fed the same chunks; one push is larger than the decoder runs in one chain"""
    raw, labels, norm, _ = recording
    probe = OnlineDecoder(engine, *norm, classes=IDS, dtype="f32")
    probe.push(raw[:2000])
    W, b, lo, span, rest = model(17, 61, host(probe.tail_view()[:64]))
    for adaptive in (False, True):
        if adaptive:
            multi = AdaptiveMultiStreamDecoder(engine, *norm, 3, 0.02, vote=9, dtype="f32", max_windows_per_push=16)
        else:
            multi = MultiStreamDecoder(engine, *norm, 3, vote=9, dtype="f32", max_windows_per_push=16)
        singles = [OnlineDecoder(engine, *norm, classes=IDS, dtype="f32", vote=9, max_windows_per_push=16, adapt=0.02 if adaptive else None)
                   for _ in range(3)]
        for s in range(3):
            multi.set_classes(s, classes=IDS)
        stage = K.JointAngles(multi, smooth=3, rate=700)
        stage.set_model(0, W, b, lo, span, rest)
        stage.set_model(2, W[:5], b[:5], lo[:5], span[:5], rest[:5])
        ones = [K.JointAngles(singles[0], smooth=3, rate=700), None, K.JointAngles(singles[2], smooth=3, rate=700)]
        ones[0].set_model(W, b, lo, span, rest)
        ones[2].set_model(W[:5], b[:5], lo[:5], span[:5], rest[:5])
        at = [0, 0, 3000]
        for sizes in ((140, 0, 333), (20, 0, 0), (500, 0, 25), (0, 0, 321)):
            chunks = [None if n == 0 else raw[a:a + n] for a, n in zip(at, sizes)]
            at = [a + n for a, n in zip(at, sizes)]
            got = stage.push(chunks)
            for s in (0, 2):
                want = ones[s].push(raw[at[s] - sizes[s]:at[s]])
                assert len(got[s]) == len(want) == 5
                for i, (g, w) in enumerate(zip(got[s], want)):
                    assert torch.equal(g, w), (adaptive, sizes, s, i)
            assert got[1][0].shape[0] == 0
        packed = stage.push_packed(torch.cat([raw[at[0]:at[0] + 100], raw[at[2]:at[2] + 60]]), [100, 0, 60])
        for s, n in ((0, 100), (2, 60)):
            want = ones[s].push(raw[at[s]:at[s] + n])
            assert all(torch.equal(g, w) for g, w in zip(packed[s], want))
        with pytest.raises(_lib.CpNativeError, match="no pose model"):
            stage.push([None, raw[:100], None])
        stage.reset([0])
        assert not stage.state(0)["out"].any() and stage.state(2)["ring"].shape[0] == 3 and multi.n_seen[0] == 0


@pytest.mark.parametrize("dtype,adapt", [("f32", None), ("bf16", 0.01)])
def test_fit_and_pick_equal_the_definitions_and_leave_the_decoder_alone(engine, recording, dtype, adapt):
    raw, labels, norm, glove = recording
    dec = OnlineDecoder(engine, *norm, classes=IDS, dtype=dtype, vote=9, adapt=adapt)
    dec.push(raw[:777])                                        # a stream in mid-flight with a filled vote ring
    expected = window_labels(labels)
    m = int(expected.shape[0])
    rep, n_rep = H.repetitions(expected)
    assert n_rep == 3
    before = dec.ws.clone(), dec.n_seen, [t.clone() for t in dec.projection()], [t.clone() for t in dec.class_table()]
    ridges, lags = [1e-2, 1.0], (0, 2)
    out = K.pick_pose(dec, raw, glove, (rep, n_rep), ridges, lags)
    fit = K.fit_pose(dec, raw, glove, rep=(rep, n_rep), ridge=[1e-2], lag=2, labels=labels, rest_label=IDS[0])
    u = dec._recording_tail_inputs(None, raw, np.arange(m))
    after = dec.ws.clone(), dec.n_seen, dec.projection(), dec.class_table()
    n_state = H._state_bytes(dec, False)                       # stream state, vote ring, the adaptive form's statistics
    assert torch.equal(before[0][:n_state], after[0][:n_state]) and before[1] == after[1] == 777
    assert all(torch.equal(a, b) for a, b in zip(before[2], after[2])) and all(torch.equal(a, b) for a, b in zip(before[3], after[3]))
    # ---- the tables against the definitions on the decoder's own tail inputs
    ref = K.pick_pose_reference(host(u), glove, (rep, n_rep), ridges, lags)
    print("mean held-out RMSE (lag, ridge):", out["rmse_mean"].tolist(), "pick", out["best"])
    assert out["sums"].shape == (2, 2, 5, 7) and out["fold_sums"].shape == (2, 3, 2, 5, 7)
    for key in ("sums", "fold_sums", "ok", "rmse", "r2", "r", "rmse_mean", "ridges", "lags"):
        assert same_bits(out[key], ref[key]), key
    assert out["best"] == ref["best"] and out["ridge"] == ref["ridge"] and out["lag"] == ref["lag"] and out["ok"].all()
    y = K.window_targets(glove, 0, 2)
    n2 = int(y.shape[0])                                       # the windows whose target, two windows on, is still inside
    assert m - 2 <= n2 < m and out["sums"][0, 0, 0, 0] == m and out["sums"][1, 0, 0, 0] == n2
    # ---- the fit against the definition
    want = K.fit_reference(host(u)[:n2], y, ridge=[1e-2], groups=rep[:n2], n_groups=3)
    assert fit.status.tolist() == [0] and fit.lag == 2 and fit.dtype == dtype and sum(fit.counts.values()) == n2
    assert same_bits(fit.W.cpu().numpy(), want["W"]) and same_bits(fit.b.cpu().numpy(), want["b"])
    lo, span, rest = K.limits(y, window_labels(labels)[:n2], IDS[0])
    assert same_bits(fit.lo, lo) and same_bits(fit.span, span) and same_bits(fit.rest, rest)
    assert same_bits(fit.apply(dec, raw).cpu().numpy()[0], K.pose_reference(host(u), want["W"][0], want["b"][0]))
    # ---- installed, the stage's raw output is the apply's
    stage = K.JointAngles(dec, fit, smooth=5)
    dec.reset()
    stage.reset()
    got = stage.push(raw[:20 * 30 + 10])
    assert got[2].shape == got[3].shape == got[4].shape == (30, 5)
    if adapt is None:                                          # (the adaptive form's statistics move with every pushed window)
        assert torch.equal(got[2], fit.apply(dec, raw)[0][:30])


def test_pick_pose_on_the_synthetic_person_equals_the_definitions():
    """`pick_pose` behind the encoder (`pick_pose_inputs`) on `kinematics_recording`, whose tail inputs lead the angles by two
    windows: every table against `pick_pose_reference`, and the held-out pick finds that lag"""
    p = K.kinematics_recording(k=4, reps=3, segment=12, joints=3, delay=2, seed=0)
    rep = (p["rep"], p["n_rep"])
    out = K.pick_pose_inputs(torch.from_numpy(p["u"]).cuda(), p["glove"], rep, [1e-2], (0, 2))
    ref = K.pick_pose_reference(p["u"], p["glove"], rep, [1e-2], (0, 2))
    assert out["sums"].shape == (2, 1, 3, 7) and out["ok"].all()
    for key in ("sums", "fold_sums", "ok", "rmse", "r2", "r", "rmse_mean", "r2_mean", "r_mean", "ridges", "lags"):
        assert same_bits(out[key], ref[key]), key
    assert out["best"] == ref["best"] == (1, 0) and out["lag"] == ref["lag"] == 2 and out["ridge"] == ref["ridge"] == 1e-2
