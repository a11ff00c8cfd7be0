"""The grasp drive on the MI355X (contrastiveprosthetics_amd/online.py GraspDrive, csrc/online_drive.cuh) against the numpy
restatement of its semantics (tests/test_online_drive_host.py DriveReference): crafted windows that make the state machine
work, cut invariance, set() between pushes, 256 streams in one launch, the copy path, and the drive behind the four decoders
wrapped in a CommandGate.  Every comparison is exact; f32 outputs are compared as bit patterns."""
import functools

import numpy as np
import pytest
import torch

from test_online_drive_host import OPEN, DriveReference, random_profile

pytestmark = pytest.mark.gpu

F = np.float32
C, ONE = 12, 4096
PARAMS = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# crafted windows
# ---------------------------------------------------------------------------------------------------------------------------
def crafted(rng, p, n, cfg, scale=1):
    """(n, 12) f32 windows and (n,) int32 class ids that walk the drive through its cases.  The profile is on a grid (rest a
    multiple of 1/64, spans powers of two, low = rest - 1, high = rest + 8) and every effort is a multiple of 1/64, so
    (x - rest) / span is exact and a window whose channels share one effort e has the level 4096 e.
    The level: holds at one effort or at one per channel, efforts below 0 and above 1 (clamped), jumps from rest to full effort
    and back (faster than rise and fall), rests, rests of `smooth` windows followed by a hold that brings the smoothed level
    to on_level exactly, stretches and short gaps without a command (-1) and with a class id the profile does not have, class changes.
    The electrodes, laid over that: a channel below low for longer and for shorter than bad_after, a channel exactly at low
    (inside), a channel that flaps above high, all channels below low at once (nothing left to sum), and NaN / inf entries."""
    ids, rest, span = np.asarray(p["ids"]), p["rest"], p["span"]
    K = len(ids)
    smooth, on = cfg["smooth"], cfg["on_level"]
    unknown = int(ids.max()) + 7
    x = np.tile(rest, (n, 1)).astype(F)
    g = np.full(n, -1, np.int32)
    plain = np.zeros(n, dtype=bool)                        # the rows of the exact approaches: no electrode trouble is laid over them
    p_exact = 0.2 if scale == 1 else 0.44                  # (a long ring needs long approaches: fewer of the other segments)

    def fill(lo, hi, k, effort):                           # effort: a multiple of 1/64, or one per channel
        hi = min(hi, n)
        if lo >= hi:
            return
        s = np.where(span[k] > 0, span[k], F(1.0))
        x[lo:hi] = rest + np.asarray(effort, dtype=F) * s
        g[lo:hi] = ids[k]

    j = 0
    while j < n:
        kind = rng.choice(["exact", "hold", "uneven", "jump", "rest", "none", "unknown", "over"],
                          p=[p_exact] + [(1 - p_exact) * q for q in (0.2, 0.2, 0.2, 0.125, 0.1, 0.0875, 0.0875)])
        k = int(rng.integers(K))
        length = int(rng.integers(5, 60)) * scale
        if kind == "hold":
            fill(j, j + length, k, rng.integers(0, 65) / 64.0)
        elif kind == "uneven":
            fill(j, j + length, k, rng.integers(0, 65, C) / 64.0)
        elif kind == "jump":                               # rest -> full -> rest, a few windows each
            third = max(length // 3, 1)
            fill(j, j + third, k, 0.0)
            fill(j + third, j + 2 * third, k, 1.0)
            fill(j + 2 * third, j + length, k, 0.0)
        elif kind == "rest":
            fill(j, j + length, k, -rng.integers(0, 9, C) / 64.0)       # at rest or a little below: clamped to 0
        elif kind == "over":
            fill(j, j + length, k, 1.0 + rng.integers(0, 17, C) / 64.0)  # above full effort: clamped to 1
        elif kind == "none":
            x[j:j + length] = rest + (rng.integers(0, 65, (min(length, n - j), C)) / 64.0).astype(F)
        elif kind == "unknown":
            fill(j, j + length, k, 1.0)
            g[j:j + length] = unknown
        else:                                              # exact: `smooth` windows of nothing, then the level that brings
            divisors = [d for d in (1, 2, 4, 5, 8, 10, 16) if smooth % d == 0 and on * d <= ONE]        # s to on_level
            d = int(rng.choice([d for d in divisors if d * 64 >= smooth] or divisors[-1:]))
            length = smooth + smooth // d + int(rng.integers(2, 8))
            fill(j, j + smooth, k, 0.0)
            fill(j + smooth, j + length, k, on * d / ONE)
            plain[j:j + length] = True
        j += length

    clean, clean_g = x.copy(), g.copy()
    j = int(rng.integers(30, 90))
    while j < n:                                           # short gaps in the command, whatever the segment
        length = int(rng.integers(3, 12))
        g[j:j + length] = -1 if rng.random() < 0.5 else unknown
        j += length + int(rng.integers(60, 240))
    bad_after, good_after = cfg["bad_after"], cfg["good_after"]
    j = int(rng.integers(20, 60))
    while j < n:
        kind = rng.choice(["long", "short", "at_low", "flap", "all"], p=[0.3, 0.2, 0.2, 0.2, 0.1])
        c = int(rng.integers(C))
        if kind == "long":
            length = bad_after + int(rng.integers(0, 2 * bad_after))
            x[j:j + length, c] = p["low"][c] - F(1.0)
        elif kind == "short":
            length = int(rng.integers(1, bad_after)) if bad_after > 1 else 0
            x[j:j + length, c] = p["low"][c] - F(1 / 64)
        elif kind == "at_low":
            length = bad_after + int(rng.integers(0, 10))
            x[j:j + length, c] = p["low"][c]
        elif kind == "flap":
            length = 0
            for _ in range(int(rng.integers(2, 6))):
                up, down = int(rng.integers(1, 2 * bad_after + 1)), int(rng.integers(1, good_after + 1))
                x[j + length:j + length + up, c] = p["high"][c] + F(rng.integers(1, 200) / 64.0)
                length += up + down
        else:
            length = bad_after + int(rng.integers(1, 12))
            x[j:j + length] = p["low"] - F(0.5)
        j += length + good_after + int(rng.integers(0, 40))
    odd = rng.random((n, C))
    x[odd < 0.002] = np.nan
    x[(odd >= 0.002) & (odd < 0.003)] = np.inf
    x[(odd >= 0.003) & (odd < 0.004)] = -np.inf
    x[plain], g[plain] = clean[plain], clean_g[plain]
    return x, g


# K, smooth, on_level, off_level, rise, fall, bad_after, good_after, rows, scale
CASES = [
    (1, 1, 512, 256, 300, 200, 6, 15, 3000, 1),
    (1, 10, 512, 256, 128, 64, 4, 9, 3000, 1),
    (2, 10, 320, 192, ONE, ONE, 6, 15, 3000, 1),
    (2, 256, 256, 128, 8, 5, 6, 15, 8000, 8),
    (41, 1, 1024, 1024, 64, ONE, 3, 5, 3000, 1),
    (41, 10, 320, 160, ONE, 100, 20, 100, 5000, 1),
    (64, 10, 0, 0, 50, 50, 6, 15, 3000, 1),                            # on_level = off_level = 0: always active
    (64, 256, 512, 64, 16, 16, 6, 15, 8000, 8),
]
SEEDS = [200, 201, 202, 203, 204, 205, 206, 207]          # chosen so that the restatement meets the coverage condition below
KEYS = ("smooth", "on_level", "off_level", "rise", "fall", "bad_after", "good_after")


def case_events(cfg):
    """the events a configuration can produce more than once: with off_level = 0 a stream never releases (and so activates
    once), and a step of 4096 is never limited"""
    ev = set(DriveReference.EVENTS)
    if cfg["off_level"] == 0:
        ev -= {"activated", "released", "at_on_level_exactly"}
    if cfg["rise"] == ONE:
        ev.discard("rise_limited")
    if cfg["fall"] == ONE:
        ev.discard("fall_limited")
    return ev


@functools.lru_cache(maxsize=None)
def case(i):
    """profile, settings, input, and the restatement's outputs, state and events: computed once, read by every test"""
    K, n, scale = CASES[i][0], CASES[i][8], CASES[i][9]
    cfg = dict(zip(KEYS, CASES[i][1:8]))
    rng = np.random.default_rng(SEEDS[i])
    p = random_profile(rng, K)
    x, g = crafted(rng, p, n, cfg, scale)
    ref = DriveReference(p, **cfg)
    want = ref.run_rows(x, g)
    for a in (x, g) + want:
        a.setflags(write=False)
    return p, cfg, x, g, want, ref.state(), dict(ref.events)


class Ids:
    """the part of a decoder that GraspDrive.apply reads: class lists (one, or one per stream) and a sample count"""
    device = torch.device("cuda:0")
    phase = 0
    vote = 25

    def __init__(self, n_streams=None):
        self.class_ids = torch.zeros(1, dtype=torch.int32) if n_streams is None else [None] * n_streams
        self.n_seen = 0 if n_streams is None else np.zeros(n_streams, dtype=np.int64)

    def push(self, *a, **k):
        raise AssertionError("apply() does not push the source")


def fractions(cfg):
    return {k: (v / ONE if k in ("on_level", "off_level", "rise", "fall") else v) for k, v in cfg.items()}


def drive_for(p, cfg):
    from contrastiveprosthetics_amd.online import GraspDrive
    return GraspDrive(Ids(), profile=p, **fractions(cfg))


def run_cuts(drive, x, g, cuts):
    xd, gd = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(g)).cuda()      # (copies: the cached inputs are read-only)
    outs, pos = [], 0
    for n in cuts:
        outs.append(drive.apply(xd[pos:pos + n], gd[pos:pos + n]))
        pos += n
    assert pos == x.shape[0]
    return [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(3)]


def assert_same(got, want, what):
    for a, w, name in zip(got, want, ("drive", "active", "bad")):
        assert a.shape == w.shape and a.dtype == w.dtype, (what, name, a.shape, w.shape, a.dtype, w.dtype)
        if a.dtype == F:                                               # bit-equal
            a, w = a.view(np.int32), w.view(np.int32)
        bad = np.nonzero(a != w)[0]
        assert bad.size == 0, (what, name, bad[:5], a[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("i", range(len(CASES)))
def test_crafted_windows_against_the_restatement(i):
    p, cfg, x, g, want, state, events = case(i)
    # the input makes the state machine work: counted on the restatement, before anything is compared
    print(CASES[i], events)
    for ev in sorted(case_events(cfg)):
        assert events[ev] >= 10, (CASES[i], ev, events)
    levels = np.rint(want[0].astype(np.float64) * ONE).astype(np.int64)
    assert levels.max() >= ONE // 2 and (levels == 0).sum() >= 100 and len(set(levels.tolist())) >= 40
    assert len(set(want[2].tolist())) >= 8 and want[2].max() == 0xfff       # several masks, and every channel bad at once
    drive = drive_for(p, cfg)
    got = run_cuts(drive, x, g, [x.shape[0]])
    assert_same(got, want, CASES[i])
    assert drive.state() == state, CASES[i]


def test_set_changes_the_settings_between_pushes():
    p, cfg, x, g, _, _, _ = case(5)
    drive = drive_for(p, cfg)
    ref = DriveReference(p, **cfg)
    got = [run_cuts(drive, x[:1500], g[:1500], [1500])]
    want = [ref.run_rows(x[:1500], g[:1500])]
    drive.set(on_level=0.25, off_level=0.125, rise=30 / ONE, fall=1.0, bad_after=3, good_after=7)
    ref.on_level, ref.off_level, ref.rise, ref.fall, ref.bad_after, ref.good_after = 1024, 512, 30, ONE, 3, 7
    got.append(run_cuts(drive, x[1500:3000], g[1500:3000], [1500]))
    want.append(ref.run_rows(x[1500:3000], g[1500:3000]))
    for a, w in zip(got, want):
        assert_same(a, w, "set")
    assert drive.state() == ref.state()
    assert ref.events["rise_limited"] > 0 and ref.events["went_bad"] > 10


@pytest.mark.parametrize("i", [1, 3, 6])
def test_outputs_and_state_do_not_depend_on_the_cut(i):
    p, cfg, x, g, want, _, _ = case(i)
    n = 1500
    x, g, want = x[:n], g[:n], [w[:n] for w in want]
    ref = DriveReference(p, **cfg)
    ref.run_rows(x, g)
    rng = np.random.default_rng(7)
    rand = []
    while sum(rand) < n:
        rand.append(int(min(rng.integers(1, 300), n - sum(rand))))
    cuts = {"1": [1] * n, "16": [16] * (n // 16) + ([n % 16] if n % 16 else []), "256": [256] * (n // 256) + [n % 256],
            "whole": [n], "random": rand, "255": [255] * (n // 255) + [n % 255]}
    states = {}
    for name, c in cuts.items():
        drive = drive_for(p, cfg)
        assert_same(run_cuts(drive, x, g, c), want, (CASES[i], name))
        assert drive.state() == ref.state(), name
        states[name] = drive.ws.cpu().numpy().copy()
    for name in cuts:
        assert np.array_equal(states[name], states["1"]), name            # the whole workspace, byte for byte


def test_256_streams_in_one_launch_each_equal_their_own_drive():
    from contrastiveprosthetics_amd.online import GraspDrive
    rng = np.random.default_rng(5)
    S, launches = 256, 12
    ks = rng.choice([1, 2, 3, 5, 17, 41, 64], S)
    cfg = dict(smooth=10, on_level=320, off_level=192, rise=200, fall=100, bad_after=4, good_after=9)
    profiles = [random_profile(rng, int(k)) for k in ks]
    many = GraspDrive(Ids(S), profile=[None if s == 9 else profiles[s] for s in range(S)], **fractions(cfg))
    m = rng.integers(0, 13, (launches, S)) * (rng.random((launches, S)) > 0.25)          # some streams sit a launch out
    m[:, 7] = 0                                                                         # one never has a row,
    m[:, 9] = 0                                                                         # and one has no profile either
    total = m.sum(axis=0)
    rows = [crafted(rng, profiles[s], int(total[s]), cfg) for s in range(S)]
    dev = [(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()) for x, g in rows]
    pos = np.zeros(S, dtype=np.int64)
    got = [[] for _ in range(S)]
    for r in range(launches):
        packed = torch.full((int(m[r].sum()), C), float("nan"), device="cuda")         # as a multi-stream push packs them
        cls = torch.full((int(m[r].sum()),), -7, dtype=torch.int32, device="cuda")
        row0 = np.concatenate([[0], np.cumsum(m[r])[:-1]])
        wv, cv = [], []
        for s in range(S):
            if m[r, s] == 0:
                wv.append(None if s % 2 else dev[s][0][:0])
                cv.append(None if s % 2 else dev[s][1][:0])
                continue
            w, c = packed[row0[s]:row0[s] + m[r, s]], cls[row0[s]:row0[s] + m[r, s]]
            w.copy_(dev[s][0][pos[s]:pos[s] + m[r, s]])
            c.copy_(dev[s][1][pos[s]:pos[s] + m[r, s]])
            wv.append(w)
            cv.append(c)
        out = many.apply(wv, cv)
        for s in range(S):
            got[s].append(out[s])
        pos += m[r]
    for s in range(S):
        a = [torch.cat([o[i] for o in got[s]]).cpu().numpy() for i in range(3)]
        ref = DriveReference(profiles[s], **cfg)
        assert_same(a, ref.run_rows(*rows[s]), ("restatement", s, int(ks[s])))
        if s == 9:
            continue
        own = drive_for(profiles[s], cfg)
        if total[s]:
            assert_same(a, run_cuts(own, rows[s][0], rows[s][1], [int(total[s])]), ("own drive", s))
        assert many.state(s) == own.state() == ref.state(), s
    assert many.state(7) == many.state(9) == dict(out=0, active=0, bad=0, run=[0] * C, ring=[])


def test_separately_allocated_windows_are_packed_for_the_launch():
    """apply() on tensors that are not one packed buffer (the caller's own) takes the copy path; a stream with rows and no
    profile is refused before anything is enqueued"""
    from contrastiveprosthetics_amd._lib import CpNativeError
    from contrastiveprosthetics_amd.online import GraspDrive
    rng = np.random.default_rng(8)
    cfg = dict(smooth=5, on_level=320, off_level=192, rise=ONE, fall=ONE, bad_after=4, good_after=9)
    profiles = [random_profile(rng, 3), None, random_profile(rng, 41)]
    drive = GraspDrive(Ids(3), profile=profiles, **fractions(cfg))
    rows = [crafted(rng, profiles[0], 700, cfg), None, crafted(rng, profiles[2], 300, cfg)]      # 700 rows: three launches
    wins = [None if r is None else torch.from_numpy(r[0]).cuda() for r in rows]
    cls = [None if r is None else torch.from_numpy(np.stack([r[1], r[1]], axis=1)).cuda()[:, 0] for r in rows]     # strided ids
    out = drive.apply(wins, cls)
    for s in (0, 2):
        ref = DriveReference(profiles[s], **cfg)
        assert_same([o.cpu().numpy() for o in out[s]], ref.run_rows(*rows[s]), s)
    assert out[1][0].shape == (0,)
    before = drive.ws.cpu().numpy().copy()
    with pytest.raises(CpNativeError, match="no drive profile"):
        drive.apply([wins[0][:5], wins[0][:5], None], [cls[0][:5].contiguous(), cls[0][:5].contiguous(), None])
    assert np.array_equal(drive.ws.cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------------------------------------
# behind the decoders
# ---------------------------------------------------------------------------------------------------------------------------
def _engine(seed=3, steps=3):
    from contrastiveprosthetics_amd.engine import Engine
    e = Engine(adabn=False, dtype="f32", device="cuda:0", seed=seed)
    e.init_parameters(seed)
    gen = torch.Generator().manual_seed(seed)
    labels = torch.arange(41).repeat(4).cuda()
    for _ in range(steps):
        x = (torch.randn(4 * 41, 12, generator=gen) * 1.5 + 0.3).cuda()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(PARAMS)
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def engine():
    return _engine()


def _recordings(n, seed=11, length=3000):
    """noise whose amplitude swells and fades, so that the windows' levels move"""
    rng = np.random.default_rng(seed)
    env = (0.3 + np.abs(np.sin(np.arange(length) / 180.0)))[:, None]
    return [torch.from_numpy((rng.standard_normal((length, 12)) * env * (1 + 0.2 * i) * 2e-3).astype(np.float32)).cuda()
            for i in range(n)]


@pytest.fixture(scope="module")
def norm():
    from contrastiveprosthetics_amd.preprocess import preprocess_segments
    rec = _recordings(1, seed=5)[0]
    w = preprocess_segments(rec[None], keep=20 * np.arange(140))[0]
    return w.mean(0), w.std(0)


def window_profile(rng, classes):
    """a profile in the units of the recordings' normalised windows (about -1.5 .. 3), not on any grid"""
    K = len(classes)
    weight = rng.integers(0, 256, (K, C)).astype(np.int32)
    span = rng.uniform(0.5, 3.0, (K, C)).astype(F)
    span[rng.random((K, C)) < 0.1] = 0
    return dict(ids=np.sort(np.asarray(classes)), rest=rng.uniform(-1.2, -0.6, C).astype(F), span=span, weight=weight,
                low=np.full(C, -1.2, F), high=np.full(C, 1.4, F))


SUBSETS = [list(range(41)), [30, 2, 17, 5, 9], [7], list(range(0, 41, 3)), [40, 0]]
CFG = dict(smooth=4, on_level=200, off_level=100, rise=400, fall=150, bad_after=2, good_after=3)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("adapt", [None, 0.01])
def test_behind_a_gated_single_decoder(engine, norm, dtype, adapt):
    from contrastiveprosthetics_amd.online import CommandGate, GraspDrive, OnlineDecoder
    mean, std = norm
    rec = _recordings(1, seed=21)[0]
    rng = np.random.default_rng(2)
    for classes, smooth in zip(SUBSETS[:3], (4, 1, 256)):
        cfg = dict(CFG, smooth=smooth)
        p = window_profile(rng, classes)
        dec = OnlineDecoder(engine, mean, std, classes=classes, vote=5, dtype=dtype, adapt=adapt)
        drive = GraspDrive(CommandGate(dec, dwell=2), profile=p, **fractions(cfg))
        opened = GraspDrive(Ids(), profile=dict(p, low=np.full(C, -np.inf, F), high=np.full(C, np.inf, F)), **fractions(OPEN))
        ref, probe = DriveReference(p, **cfg), DriveReference(p, **OPEN)
        pos, n_rows = 0, 0
        while pos < rec.shape[0]:
            n = int(rng.integers(1, 700))
            out = drive.push(rec[pos:pos + n], return_windows=True)
            assert len(out) == 10
            pred, voted, wins, cmd = out[:4]
            want = ref.run_rows(wins.cpu().numpy(), cmd.cpu().numpy())
            assert_same([o.cpu().numpy() for o in out[7:]], want, (classes, pos))
            # every gate open: the level of each window on its own
            raw = np.array([probe.raw_level(w, int(c)) for w, c in zip(wins.cpu().numpy(), cmd.cpu().numpy())], dtype=np.int64)
            level = opened.apply(wins, cmd)[0].cpu().numpy()
            assert np.array_equal(level.view(np.int32), (raw.astype(F) / F(ONE)).view(np.int32))
            assert len(drive.push(rec[:0])) == 9                       # an empty push: empty outputs, the windows dropped
            pos += n
            n_rows += pred.shape[0]
        assert n_rows == 150 and drive.state() == ref.state()
        assert ref.events["went_bad"] > 0 and ref.events["activated"] > 0 and ref.events["clamped_low"] > 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("adaptive", [False, True])
def test_behind_a_gated_multi_decoder(engine, norm, dtype, adaptive):
    from contrastiveprosthetics_amd.online import AdaptiveMultiStreamDecoder, CommandGate, GraspDrive, MultiStreamDecoder
    mean, std = norm
    S = len(SUBSETS) + 1                                               # the last stream never gets classes, profile or samples
    recs = _recordings(S - 1, seed=31)
    if adaptive:
        dec = AdaptiveMultiStreamDecoder(engine, mean, std, S, [0.0, 0.01, 0.02, 0.0, 0.05, 0.01], vote=9, dtype=dtype)
    else:
        dec = MultiStreamDecoder(engine, mean, std, S, vote=9, dtype=dtype, max_windows_per_push=16, max_rows=40)
    for s, classes in enumerate(SUBSETS):
        dec.set_classes(s, classes=classes)
    rng = np.random.default_rng(3)
    profiles = [window_profile(rng, c) for c in SUBSETS]
    drive = GraspDrive(CommandGate(dec, dwell=2), profile=profiles + [None], **fractions(CFG))
    refs = [DriveReference(p, **CFG) for p in profiles]
    pos = np.zeros(S - 1, dtype=np.int64)
    rows = 0
    while (pos < 3000).any():
        n = np.minimum(rng.integers(1, 500, S - 1) * (rng.random(S - 1) > 0.3), 3000 - pos)      # (the small decoder splits these)
        chunks = [recs[s][pos[s]:pos[s] + n[s]] if n[s] or s % 2 else None for s in range(S - 1)] + [None]
        out = drive.push(chunks, return_windows=True)
        for s in range(S - 1):
            assert len(out[s]) == 10
            wins, cmd = out[s][2], out[s][3]
            assert_same([o.cpu().numpy() for o in out[s][7:]], refs[s].run_rows(wins.cpu().numpy(), cmd.cpu().numpy()), (s, pos))
            rows += wins.shape[0]
        assert out[S - 1][7].shape == (0,)
        pos += n
    assert rows == 150 * (S - 1)
    assert all(drive.state(s) == refs[s].state() for s in range(S - 1))
    raw = torch.cat([r[:60] for r in recs])
    drive.reset()
    assert dec.n_seen.sum() == 0 and drive.state(1) == dict(out=0, active=0, bad=0, run=[0] * C, ring=[])
    out = drive.push_packed(raw, [60] * (S - 1) + [0], return_logits=True)
    assert all(len(o) == 10 and o[2].shape[1] == len(c) and o[7].shape == o[0].shape == (3,) for o, c in zip(out, SUBSETS))


def test_follows_the_source_and_refuses_a_push_behind_its_back(engine, norm):
    from contrastiveprosthetics_amd._lib import CpNativeError
    from contrastiveprosthetics_amd.online import CommandGate, GraspDrive, OnlineDecoder
    mean, std = norm
    rec = _recordings(1, seed=41)[0]
    rng = np.random.default_rng(4)
    p = window_profile(rng, [3, 8, 20])
    cfg = dict(CFG, on_level=0, off_level=0, bad_after=65535)          # always active, every channel good
    dec = OnlineDecoder(engine, mean, std, classes=[3, 8, 20], vote=25)
    drive = GraspDrive(dec, profile=p, **fractions(cfg))               # behind a decoder: follows voted
    assert drive.follow == "voted"
    ref = DriveReference(p, **cfg)
    pred, voted, wins, level, active, bad = drive.push(rec[:1000], return_windows=True)
    assert_same([level.cpu().numpy(), active.cpu().numpy(), bad.cpu().numpy()], ref.run_rows(wins.cpu().numpy(), voted.cpu().numpy()), "voted")
    assert float(level.max()) > 0
    by_pred = GraspDrive(Ids(), profile=p, follow="pred", **fractions(cfg))
    assert by_pred.follow == "pred"
    dec.set_classes([2, 4, 6])                                         # none of them in the profile: the level falls to 0
    out = drive.push(rec[1000:2000])
    assert len(out) == 5 and float(out[2][-1]) == 0.0 and drive.state()["ring"] == [0] * 4
    dec.set_classes([3, 8, 20])
    drive.push(rec[2000:2400])
    assert drive.state()["out"] > 0
    drive.set_profile(window_profile(rng, [3, 8, 20]))                 # a new profile: the stream starts again
    assert drive.state() == dict(out=0, active=0, bad=0, run=[0] * C, ring=[])
    drive.push(rec[2400:2500])
    assert len(drive.state()["ring"]) == 4
    drive.reset()
    assert dec.n_seen == 0 and drive.state() == dict(out=0, active=0, bad=0, run=[0] * C, ring=[])
    gate = CommandGate(dec, dwell=2)
    drive = GraspDrive(gate, profile=p, **fractions(cfg))
    assert drive.follow == "command"
    drive.push(rec[:500])
    gate.push(rec[500:520])                                            # behind the drive's back
    before = drive.ws.cpu().numpy().copy()
    with pytest.raises(CpNativeError, match="behind"):
        drive.push(rec[520:600])
    assert dec.n_seen == 520 and np.array_equal(drive.ws.cpu().numpy(), before)      # nothing was enqueued
    drive.reset()
    assert gate.state() == dict(command=-1, pending=None, run=0, ring=[])
    assert len(drive.push(rec[:100])[6]) == 5
    bare = GraspDrive(OnlineDecoder(engine, mean, std, classes=[3, 8, 20]))
    with pytest.raises(CpNativeError, match="no drive profile"):
        bare.push(rec[:100])
    assert bare.decoder.n_seen == 0
