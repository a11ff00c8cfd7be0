"""CPU checks of the grasp drive (contrastiveprosthetics_amd/online.py GraspDrive, csrc/online_drive.cuh): the numpy
restatement of its semantics that the GPU tests compare against (`DriveReference`) with checks of the restatement itself, the
C ABI against the header, the refusals of the cp_online_drive_* entries before any device call, and `drive_profile` on a
synthetic cued recording."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
DRIVE = ["cp_online_drive_workspace_bytes", "cp_online_drive_set_profile", "cp_online_drive_reset", "cp_online_drive_push"]
ERR_ARG = 10001
F = np.float32
C, ONE = 12, 4096


# ---------------------------------------------------------------------------------------------------------------------------
# the semantics of include/cpnative.h, restated: one stream, one window at a time, single f32 operations, integer levels
# ---------------------------------------------------------------------------------------------------------------------------
class DriveReference:
    """One stream of the drive.  Levels are integers out of 4096.  `events` counts what the state machine did, so that a test
    can show its input made it work."""
    EVENTS = ("went_bad", "recovered", "activated", "released", "rise_limited", "fall_limited", "no_command", "unknown_class",
              "no_usable_channel", "clamped_low", "clamped_high", "nonfinite", "at_low_exactly", "at_on_level_exactly")

    def __init__(self, profile, smooth=10, on_level=328, off_level=164, rise=ONE, fall=ONE, bad_after=20, good_after=100):
        self.smooth = int(smooth)
        self.on_level, self.off_level, self.rise, self.fall = int(on_level), int(off_level), int(rise), int(fall)
        self.bad_after, self.good_after = int(bad_after), int(good_after)
        assert 1 <= self.smooth <= 256 and 0 <= self.off_level <= self.on_level <= ONE
        self.events = dict.fromkeys(self.EVENTS, 0)
        self.set_profile(profile)

    def set_profile(self, p):
        self.ids = [int(i) for i in p["ids"]]
        K = len(self.ids)
        assert self.ids == sorted(set(self.ids)) and self.ids[0] >= 0 and 1 <= K <= 64
        self.rest, self.low, self.high = (np.asarray(p[k], dtype=F).reshape(C).copy() for k in ("rest", "low", "high"))
        self.span = np.asarray(p["span"], dtype=F).reshape(K, C).copy()
        self.weight = np.asarray(p["weight"], dtype=np.int64).reshape(K, C).copy()
        assert self.weight.min() >= 0 and self.weight.max() <= 255
        self.reset()

    def reset(self):
        self.is_bad = [False] * C
        self.run = [0] * C
        self.ring = []                           # raw levels, oldest first
        self.active, self.out = 0, 0

    def bad_mask(self):
        return sum(1 << c for c in range(C) if self.is_bad[c])

    def state(self):
        return dict(out=self.out, active=self.active, bad=self.bad_mask(), run=list(self.run), ring=list(self.ring))

    def raw_level(self, x, g):
        """step 2 on its own, with the present status of the channels"""
        ev = self.events
        if g == -1:
            ev["no_command"] += 1
            return 0
        if g not in self.ids:
            ev["unknown_class"] += 1
            return 0
        k = self.ids.index(g)
        swq = sw = 0
        with np.errstate(all="ignore"):
            for c in range(C):
                w, span = int(self.weight[k, c]), self.span[k, c]
                if not (w > 0 and span > F(0)) or self.is_bad[c]:
                    continue
                e = F(F(x[c] - self.rest[c]) / span)
                ev["clamped_low"] += bool(e < F(0))
                ev["clamped_high"] += bool(e > F(1))
                a = np.fmin(np.fmax(e, F(0)), F(1))                  # fmax / fmin: NaN -> 0
                q = int(np.rint(F(a * F(ONE))))
                swq += w * q
                sw += w
        if sw == 0:
            ev["no_usable_channel"] += 1
            return 0
        return swq // sw

    def step(self, x, g):
        """x (12,) f32, g a class id or -1 -> (drive f32, active, bad)"""
        x = np.asarray(x, dtype=F)
        assert x.shape == (C,)
        ev = self.events
        # 1. health
        for c in range(C):
            ev["nonfinite"] += not np.isfinite(x[c])
            ev["at_low_exactly"] += bool(x[c] == self.low[c])
            inside = bool(np.isfinite(x[c]) and x[c] >= self.low[c] and x[c] <= self.high[c])
            if inside == self.is_bad[c]:                             # a good channel outside, or a bad one inside
                self.run[c] += 1
            else:
                self.run[c] = 0
            if self.run[c] >= (self.good_after if self.is_bad[c] else self.bad_after):
                ev["recovered" if self.is_bad[c] else "went_bad"] += 1
                self.is_bad[c] = not self.is_bad[c]
                self.run[c] = 0
        bad = self.bad_mask()
        # 2. raw level
        raw = self.raw_level(x, int(g))
        # 3. smooth
        self.ring.append(raw)
        if len(self.ring) > self.smooth:
            self.ring.pop(0)
        s = sum(self.ring) // len(self.ring)
        # 4. hysteresis
        if not self.active and s >= self.on_level:
            ev["activated"] += 1
            ev["at_on_level_exactly"] += s == self.on_level
            self.active = 1
        elif self.active and s < self.off_level:
            ev["released"] += 1
            self.active = 0
        # 5. slew
        target = s if self.active else 0
        if target > self.out:
            ev["rise_limited"] += target > self.out + self.rise
            self.out = min(self.out + self.rise, target)
        else:
            ev["fall_limited"] += target < self.out - self.fall
            self.out = max(self.out - self.fall, target)
        return F(self.out) / F(ONE), self.active, bad

    def run_rows(self, windows, cls):
        """(M, 12) f32, (M,) -> drive (M,) f32, active, bad (M,) int32"""
        out = [self.step(x, g) for x, g in zip(np.asarray(windows, dtype=F), np.asarray(cls))]
        if not out:
            return np.zeros(0, F), np.zeros(0, np.int32), np.zeros(0, np.int32)
        d, a, b = zip(*out)
        return np.array(d, F), np.array(a, np.int32), np.array(b, np.int32)


OPEN = dict(smooth=1, on_level=0, off_level=0, rise=ONE, fall=ONE)


def random_profile(rng, K, grid=True, open_range=False):
    """a profile on a grid of 1/64 (every (x - rest) / span the tests craft is then exact): spans of 0.5, 1, 2 or 4, some channels
    unused (weight 0, span 0 or negative)"""
    ids = np.sort(rng.choice(500, K, replace=False)).astype(np.int64)
    rest = (rng.integers(-32, 32, C) / 64.0).astype(F)
    span = rng.choice([0.5, 1.0, 2.0, 4.0], (K, C)).astype(F)
    weight = rng.integers(1, 256, (K, C))
    off = rng.random((K, C))
    weight[off < 0.15] = 0
    span[(off >= 0.15) & (off < 0.25)] = 0
    span[(off >= 0.25) & (off < 0.3)] = -1.0
    if not grid:
        rest = rng.normal(0, 0.3, C).astype(F)
        span = np.where(span > 0, rng.uniform(0.3, 5.0, (K, C)), span).astype(F)
    low = np.full(C, -np.inf, F) if open_range else (rest - F(1.0)).astype(F)
    high = np.full(C, np.inf, F) if open_range else (rest + F(8.0)).astype(F)
    return dict(ids=ids, rest=rest, span=span, weight=weight.astype(np.int32), low=low, high=high)


def random_rows(rng, p, n):
    K = len(p["ids"])
    x = (p["rest"] + rng.uniform(-0.5, 3.0, (n, C))).astype(F)
    x[rng.random((n, C)) < 0.01] = np.nan
    g = np.array(p["ids"])[rng.integers(K, size=n)]
    g[rng.random(n) < 0.1] = -1
    g[rng.random(n) < 0.05] = 501
    return x, g.astype(np.int32)


def test_reference_open_setting_gives_the_raw_level():
    rng = np.random.default_rng(0)
    for K in (1, 2, 41, 64):
        p = random_profile(rng, K, grid=False, open_range=True)
        x, g = random_rows(rng, p, 300)
        ref = DriveReference(p, **OPEN)
        probe = DriveReference(p, **OPEN)
        drive, active, bad = ref.run_rows(x, g)
        raw = np.array([probe.raw_level(xi, int(gi)) for xi, gi in zip(x, g)])
        assert np.array_equal(drive.view(np.int32), (raw.astype(F) / F(ONE)).view(np.int32))
        assert (bad == 0).all() and (active == 1).all()
        assert raw.max() > 3000 and raw.min() == 0 and len(set(raw.tolist())) > 100
        assert ref.events["went_bad"] == 0 and ref.events["rise_limited"] == 0 and ref.events["fall_limited"] == 0
        assert ref.events["no_command"] > 0 and ref.events["unknown_class"] > 0 and ref.events["nonfinite"] > 0


def test_reference_raw_level_by_hand():
    p = dict(ids=[4, 9], rest=np.full(C, 0.25, F), span=np.ones((2, C), F), weight=np.zeros((2, C), np.int32),
             low=np.full(C, -np.inf, F), high=np.full(C, np.inf, F))
    p["weight"][1, 0], p["weight"][1, 1], p["weight"][1, 2] = 1, 3, 200
    p["span"][1, 1] = 2.0
    p["span"][1, 2] = np.nan                                          # a NaN span: the channel is not used
    ref = DriveReference(p, **OPEN)
    x = np.full(C, 0.25, F)
    x[0], x[1] = 0.75, 1.25                                           # a = 0.5 and 0.5: q = 2048 each
    assert ref.step(x, 9) == (F(0.5), 1, 0)
    x[1] = np.nan                                                     # NaN -> 0: (1 * 2048 + 3 * 0) // 4
    assert ref.step(x, 9)[0] == F(512) / F(ONE)
    x[1] = np.inf                                                     # clamped to 1: (2048 + 3 * 4096) // 4 = 3584
    assert ref.step(x, 9)[0] == F(3584) / F(ONE)
    assert ref.step(x, 4)[0] == 0 and ref.events["no_usable_channel"] == 1       # class 4 has no weights
    assert ref.step(x, -1)[0] == 0 and ref.step(x, 5)[0] == 0
    assert ref.events["no_command"] == 1 and ref.events["unknown_class"] == 1


def test_reference_does_not_depend_on_the_cut():
    rng = np.random.default_rng(1)
    p = random_profile(rng, 5)
    x, g = random_rows(rng, p, 700)
    x[200:260, 3] = p["rest"][3] - F(2.0)                             # a channel at the floor, then back
    cfg = dict(smooth=7, on_level=900, off_level=500, rise=300, fall=150, bad_after=5, good_after=9)
    whole = DriveReference(p, **cfg)
    want = whole.run_rows(x, g)
    assert whole.events["went_bad"] >= 1 and whole.events["recovered"] >= 1 and want[2].max() == 8
    for step in (1, 16, 255, 333):
        ref = DriveReference(p, **cfg)
        parts = [ref.run_rows(x[i:i + step], g[i:i + step]) for i in range(0, 700, step)]
        for i in range(3):
            got = np.concatenate([q[i] for q in parts])
            assert np.array_equal(got.view(np.int32), want[i].view(np.int32)), (step, i)
        assert ref.state() == whole.state()


def test_reference_channel_outside_for_less_than_bad_after_stays_good():
    p = random_profile(np.random.default_rng(2), 2)
    x = np.tile(p["rest"] + F(0.5), (100, 1)).astype(F)
    g = np.full(100, p["ids"][0], np.int32)
    x[10:10 + 7, 5] = p["low"][5] - F(0.25)                           # bad_after - 1 windows outside: stays good
    x[40:40 + 8, 5] = np.nan                                          # bad_after windows: bad from the eighth on
    x[60:, 5] = p["low"][5]                                           # exactly at low is inside
    ref = DriveReference(p, bad_after=8, good_after=30)
    bad = ref.run_rows(x, g)[2]
    assert (bad[:47] == 0).all() and (bad[47:77] == 1 << 5).all() and (bad[77:] == 0).all()
    assert ref.events["went_bad"] == 1 and ref.events["recovered"] == 1 and ref.events["at_low_exactly"] == 40


def test_reference_out_moves_by_at_most_rise_and_fall():
    rng = np.random.default_rng(3)
    p = random_profile(rng, 3)
    x, g = random_rows(rng, p, 1500)
    ref = DriveReference(p, smooth=3, on_level=400, off_level=200, rise=37, fall=91)
    drive = ref.run_rows(x, g)[0]
    out = np.concatenate([[0], np.rint(drive.astype(np.float64) * ONE).astype(np.int64)])
    d = np.diff(out)
    assert d.max() <= 37 and d.min() >= -91 and d.max() == 37 and d.min() == -91
    assert ref.events["rise_limited"] > 10 and ref.events["fall_limited"] > 10


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


FIELDS = ["smooth", "on_level", "off_level", "rise", "fall", "bad_after", "good_after"]


def test_drive_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in DRIVE:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    body = hdr[hdr.index("typedef struct cp_online_drive_config {"):hdr.index("} cp_online_drive_config;")]
    fields = re.findall(r"\bint32_t\s+(\w+);", body)
    assert fields == [f[0] for f in _lib.cp_online_drive_config._fields_] == FIELDS
    assert all(f[1] is ctypes.c_int32 for f in _lib.cp_online_drive_config._fields_)
    assert ctypes.sizeof(_lib.cp_online_drive_config) == 28
    for name, value in (("CP_ONLINE_DRIVE_ONE", ONE), ("CP_ONLINE_DRIVE_MAX_SMOOTH", 256)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == value == getattr(_lib, name)
    from contrastiveprosthetics_amd import online
    assert online.DRIVE_ONE == ONE


def test_drive_workspace_grows_linearly_in_the_streams(lib):
    one = lib.cp_online_drive_workspace_bytes(1)
    # K, head, len, active, out, bad, run[12], ids[64], rest, low, high [12], span [64][12] f32, weight [64][12] bytes, ring [256]
    assert one >= 4 * (6 + 12 + 64 + 36 + 768 + 256) + 768 and one % 256 == 0
    per = (lib.cp_online_drive_workspace_bytes(256) - lib.cp_online_drive_workspace_bytes(128)) // 128
    for s in (2, 3, 64, 255, 256):
        got = lib.cp_online_drive_workspace_bytes(s)
        assert got % 256 == 0 and s * per <= got < s * per + 256, s
    assert lib.cp_online_drive_workspace_bytes(0) == one
    from contrastiveprosthetics_amd import online
    assert per == 4 * online._OD_WORDS                                 # what GraspDrive.state reads back


def _dcfg(**kw):
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_drive_config()
    cfg.smooth, cfg.on_level, cfg.off_level, cfg.rise, cfg.fall, cfg.bad_after, cfg.good_after = 10, 328, 164, ONE, ONE, 20, 100
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_drive_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory as the 'workspace': every refusal returns before a launch, which on this machine would fail differently"""
    S = 4
    need = lib.cp_online_drive_workspace_bytes(S)
    buf = ctypes.create_string_buffer(need + 256)
    ws = (ctypes.addressof(buf) + 255) // 256 * 256
    ids = (ctypes.c_int32 * 65)(*range(65))
    chan = (ctypes.c_float * 12)()
    lo = (ctypes.c_float * 12)(*[-1.0] * 12)
    hi = (ctypes.c_float * 12)(*[1.0] * 12)
    span = (ctypes.c_float * (65 * 12))()
    weight = (ctypes.c_int32 * (65 * 12))()
    rows = (ctypes.c_int32 * S)()
    out = (ctypes.c_int32 * 8)()
    fout = (ctypes.c_float * 8)()
    win = (ctypes.c_float * 64)()
    sp, rs, pu = "cp_online_drive_set_profile", "cp_online_drive_reset", "cp_online_drive_push"

    def calls(cfg, n_streams=S, w=ws, nbytes=need):
        cr = ctypes.byref(cfg)
        return ((sp, lambda: lib.cp_online_drive_set_profile(cr, n_streams, w, nbytes, 0, ids, 2, chan, span, weight, lo, hi, None)),
                (rs, lambda: lib.cp_online_drive_reset(cr, n_streams, w, nbytes, -1, None)),
                (pu, lambda: lib.cp_online_drive_push(cr, n_streams, w, nbytes, win, 12, out, rows, rows, 1, fout, out, out, None)))

    def err(rc, entry, what):
        assert rc == ERR_ARG, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    def each(cfg, what, **kw):                      # every entry refuses, one at a time (cp_last_error is the last call's)
        for entry, call in calls(cfg, **kw):
            err(call(), entry, what)

    each(_dcfg(smooth=0), "smooth")
    each(_dcfg(smooth=257), "smooth")
    each(_dcfg(on_level=-1, off_level=-1), "on_level")
    each(_dcfg(on_level=ONE + 1), "on_level")
    each(_dcfg(off_level=-1), "off_level")
    each(_dcfg(off_level=ONE + 1, on_level=ONE), "off_level")
    each(_dcfg(on_level=100, off_level=101), "off_level must not exceed on_level")
    each(_dcfg(rise=0), "rise")
    each(_dcfg(rise=ONE + 1), "rise")
    each(_dcfg(fall=0), "fall")
    each(_dcfg(fall=ONE + 1), "fall")
    each(_dcfg(bad_after=0), "bad_after")
    each(_dcfg(bad_after=65536), "bad_after")
    each(_dcfg(good_after=0), "good_after")
    each(_dcfg(good_after=65536), "good_after")
    each(_dcfg(), "n_streams", n_streams=0)
    each(_dcfg(), "n_streams", n_streams=257)
    each(_dcfg(), "workspace", w=None)
    each(_dcfg(), "workspace", w=ws + 4)
    each(_dcfg(), "workspace", nbytes=need - 257)                          # a short workspace
    each(_dcfg(), "workspace", n_streams=S + 1)                            # sized for fewer streams
    cfg = _dcfg()
    cr = ctypes.byref(cfg)

    def prof(index=0, i=ids, k=2, r=chan, s=span, w=weight, l=lo, h=hi):
        return lib.cp_online_drive_set_profile(cr, S, ws, need, index, i, k, r, s, w, l, h, None)

    err(prof(k=0), sp, "classes")
    err(prof(k=65), sp, "classes")
    err(prof(i=None), sp, "classes")
    err(prof(s=None), sp, "classes")
    err(prof(index=S), sp, "stream index")
    err(prof(index=-1), sp, "stream index")
    for bad in ([3, 2], [2, 2], [-1, 4]):                                 # unsorted, repeated, negative (-1 is 'none')
        err(prof(i=(ctypes.c_int32 * 2)(*bad)), sp, "ascending")
    err(prof(r=(ctypes.c_float * 12)(*[0.0] * 11 + [float("nan")])), sp, "rest")
    err(prof(r=(ctypes.c_float * 12)(*[0.0] * 11 + [float("inf")])), sp, "rest")
    err(prof(l=(ctypes.c_float * 12)(*[0.0] * 11 + [float("nan")])), sp, "low")
    err(prof(l=(ctypes.c_float * 12)(*[0.0] * 11 + [2.0])), sp, "low")    # above high
    err(prof(w=(ctypes.c_int32 * 24)(*[0] * 23 + [256])), sp, "weight")
    err(prof(w=(ctypes.c_int32 * 24)(*[0] * 23 + [-1])), sp, "weight")
    err(lib.cp_online_drive_reset(cr, S, ws, need, S, None), rs, "stream index")
    err(lib.cp_online_drive_reset(cr, S, ws, need, -2, None), rs, "stream index")

    def push(w=win, ldw=12, c=out, r0=rows, m=rows, total=1, d=fout, a=out, b=out):
        return lib.cp_online_drive_push(cr, S, ws, need, w, ldw, c, r0, m, total, d, a, b, None)

    err(push(total=65537), pu, "total_rows")
    err(push(total=-1), pu, "total_rows")
    err(push(ldw=11), pu, "ldw")
    err(push(w=None), pu, "windows")
    err(push(c=None), pu, "cls")
    err(push(r0=None), pu, "row0")
    err(push(m=None), pu, "row0")
    err(push(d=None), pu, "drive")
    err(push(b=None), pu, "bad")
    err(push(w=ctypes.addressof(win) + 2), pu, "misaligned")
    assert lib.cp_online_drive_push(cr, S, ws, need, None, 12, None, None, None, 0, None, None, None, None) == 0     # nothing to do


def test_wrapper_refuses_bad_settings_and_profiles_on_the_host():
    """GraspDrive checks its settings and profiles before it loads the library or touches the device"""
    import torch
    from contrastiveprosthetics_amd.online import GraspDrive, _check_profile

    class Stub:
        class_ids = torch.tensor([1, 4], dtype=torch.int32)
        n_seen, vote, phase = 0, 25, 0

        def push(self, *a, **k):
            raise AssertionError("not pushed")

    d = GraspDrive(Stub())
    assert d.follow == "voted" and not d.multi and d.ws is None
    c = d._cfg
    assert (c.smooth, c.on_level, c.off_level, c.rise, c.fall, c.bad_after, c.good_after) == (10, 328, 164, ONE, ONE, 20, 100)
    d.set(on_level=0.5, off_level=0.25, rise=0.125, fall=1 / ONE)
    assert (c.on_level, c.off_level, c.rise, c.fall) == (2048, 1024, 512, 1)
    for kw in (dict(smooth=5), dict(on_level=1.5), dict(off_level=0.75), dict(rise=0.0), dict(fall=0.0001), dict(bad_after=0),
               dict(good_after=65536), dict(bad_after=2.5), dict(on_level=True)):
        with pytest.raises(ValueError):
            d.set(**kw)
    assert (c.on_level, c.off_level, c.rise, c.fall, c.bad_after, c.good_after) == (2048, 1024, 512, 1, 20, 100)
    with pytest.raises(TypeError):
        d.set(dwell=3)
    for kw in (dict(smooth=0), dict(smooth=257), dict(follow="command"), dict(follow="best"), dict(off_level=0.5)):
        with pytest.raises(ValueError):
            GraspDrive(Stub(), **kw)
    with pytest.raises(TypeError):
        GraspDrive(object())
    with pytest.raises(TypeError):
        d.set_profile(0, {})
    p = random_profile(np.random.default_rng(4), 3)
    assert _check_profile(p)["weight"].dtype == np.int32
    for key, value in (("rest", np.full(C, np.nan)), ("low", p["high"] + 1), ("weight", p["weight"] + 256),
                       ("weight", p["weight"].astype(F)), ("span", p["span"][:2]), ("ids", p["ids"][::-1])):
        with pytest.raises(ValueError):
            _check_profile({**p, key: value})
    with pytest.raises(ValueError):
        _check_profile({k: v for k, v in p.items() if k != "low"})


# ---------------------------------------------------------------------------------------------------------------------------
# drive_profile
# ---------------------------------------------------------------------------------------------------------------------------
def _cued_recording(rng):
    """rest around a per-channel level, three classes that each raise their own channels, one class with too few windows"""
    from contrastiveprosthetics_amd.online import IGNORE, REST
    rest_level = rng.uniform(-1.2, -0.8, C)
    gains = {3: np.zeros(C), 7: np.zeros(C), 20: np.zeros(C), 31: np.zeros(C)}
    gains[3][:4] = [2.0, 1.0, 0.5, 0.25]
    gains[7][4:8] = [1.0, 3.0, 1.0, 0.25]
    gains[20][8:] = [0.5, 0.5, 4.0, 1.0]
    gains[31][:] = 1.0
    rows, exp = [], []
    for _ in range(6):
        for c, n in ((REST, 80), (3, 60), (IGNORE, 10), (7, 60), (REST, 40), (20, 60), (31, 3)):
            base = rest_level + rng.normal(0, 0.02, (n, C))
            if c >= 0:
                base = base + gains[c] * rng.uniform(0.3, 1.0, (n, 1))
            if c == IGNORE:
                base = base + 50.0                                   # a transition the cue does not score: not "seen"
            rows.append(base)
            exp.append(np.full(n, c))
    return np.concatenate(rows).astype(F), np.concatenate(exp), rest_level, gains


def test_drive_profile_from_a_synthetic_cued_recording():
    from contrastiveprosthetics_amd.online import REST, _check_profile, drive_profile
    rng = np.random.default_rng(6)
    w, e, rest_level, gains = _cued_recording(rng)
    ids = [3, 7, 20, 31, 40]                                           # 31: 18 windows; 40: never cued
    floor = np.full(C, -3.0)
    p = drive_profile(w, e, ids, level=0.9, floor=floor, min_windows=25, headroom=4.0)
    assert p["ids"].tolist() == ids
    w64 = w.astype(np.float64)
    rest = np.median(w64[e == REST], axis=0)
    assert np.array_equal(p["rest"], rest.astype(F)) and np.abs(p["rest"] - rest_level).max() < 0.01
    for k, c in enumerate(ids[:3]):
        span = np.quantile(w64[e == c], 0.9, axis=0) - rest
        assert np.array_equal(p["span"][k], span.astype(F))
        on = gains[c] > 0
        assert (p["span"][k][on] > 0.15).all() and (np.abs(p["span"][k][~on]) < 0.05).all()     # (off: the noise's quantile)
        assert np.array_equal(p["weight"][k], np.rint(255 * np.maximum(span, 0) / span.max()).astype(np.int32))
        assert p["weight"][k].max() == 255 and p["weight"][k].argmax() == gains[c].argmax()
        assert (p["weight"][k][~on] <= 6).all()
    assert (p["span"][3:] == 0).all() and (p["weight"][3:] == 0).all()     # under min_windows, and never cued
    assert (p["low"] < p["rest"]).all() and (p["rest"] < p["high"]).all()
    seen = w64[e != -2]
    assert np.array_equal(p["high"], (rest + 4.0 * (seen.max(axis=0) - rest)).astype(F)) and (p["high"] < 40).all()
    assert np.array_equal(p["low"], (0.5 * (floor + seen.min(axis=0))).astype(F))
    assert (drive_profile(w, e, ids)["low"] == -np.inf).all()
    assert (drive_profile(w, e, ids, min_windows=10)["span"][3] > 0).all()
    _check_profile(p)
    # the profile does what it is for: full effort of a class drives near 1, rest drives 0
    ref = DriveReference(p, **OPEN)
    full = (rest + np.maximum(p["span"][1], 0)).astype(F)
    assert ref.step(full, 7)[0] >= F(0.99) and ref.step(rest.astype(F), 7)[0] <= F(0.01)
    with pytest.raises(ValueError, match="REST"):
        drive_profile(w[e != REST], e[e != REST], ids)
    with pytest.raises(ValueError):
        drive_profile(w, e[:-1], ids)
    with pytest.raises(ValueError):
        drive_profile(w, e, ids, level=0.0)
