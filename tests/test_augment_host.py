"""CPU-only checks of the gather augmentation: the cp_augment / cp_step_state layouts against include/cpnative.h,
every refusal of cp_gather_groups_aug (host-only: each returns before anything is enqueued, the device pointers are dummy
addresses that are never dereferenced), every Augment validation error, and the statistics of the draws that
augment.Augment.reference -- the numpy definition of the kernel -- is made of."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def header_fields(struct):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = hdr[hdr.index("typedef struct %s {" % struct) + len("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.search(r"(\w+)\s*(\[\d+\])?$", first.strip()).group(1))
        names += [r.strip().lstrip("*").split("[")[0] for r in rest]
    return names


def test_struct_layouts_match_header():
    from contrastiveprosthetics_amd import _lib
    assert header_fields("cp_augment") == [f[0] for f in _lib.cp_augment._fields_]
    assert ctypes.sizeof(_lib.cp_augment) == 4 * 4 + 2 * 4 + 4 + 5 * 4 + 8 + 8 == 64
    assert _lib.cp_augment.mean_std.offset == 48 and _lib.cp_augment.item_offset.offset == 56
    # cp_step_state keeps its 32 bytes: the salt took the first of the three pad words (word 5)
    assert header_fields("cp_step_state") == [f[0] for f in _lib.cp_step_state._fields_]
    assert ctypes.sizeof(_lib.cp_step_state) == 32
    assert _lib.cp_step_state.aug_salt.offset == 20 and _lib.cp_step_state.lr_glove.offset == 16
    assert "cp_gather_groups_aug" in _lib.SYMBOLS


def good(_lib, **over):
    a = _lib.cp_augment()
    a.seed, a.salt, a.shift_min, a.shift_max = 1, 2, -1, 1
    a.p_drop, a.gain_sigma, a.amp_sigma, a.noise_sigma, a.fill = 0.1, 0.3, 0.2, 0.05, 0.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_entry_refuses_bad_settings_before_it_launches(lib):
    from contrastiveprosthetics_amd import _lib
    ok = 0x100000                                                 # a 16-byte aligned dummy address
    nan, inf = float("nan"), float("inf")

    def call(aug, B=2, table=ok, out=ok):
        return lib.cp_gather_groups_aug(table, 41 * 50, ok, 50, ok, B, 1, out, ctypes.byref(aug) if aug is not None else None, None)

    cases = [("NULL aug", None, {}),
             ("shift_min = -8", good(_lib, shift_min=-8), {}),
             ("shift_max = 8", good(_lib, shift_max=8), {}),
             ("shift_min > shift_max", good(_lib, shift_min=2, shift_max=1), {}),
             ("p_drop < 0", good(_lib, p_drop=-0.01), {}),
             ("p_drop > 1", good(_lib, p_drop=1.01), {}),
             ("p_drop NaN", good(_lib, p_drop=nan), {}),
             ("dead_mask bit 12", good(_lib, dead_mask=0x1000), {}),
             ("fill inf", good(_lib, fill=inf), {}),
             ("fill NaN", good(_lib, fill=nan), {}),
             ("item_offset < 0", good(_lib, item_offset=-1), {}),
             ("item_offset + B * 41 = 2^32 + 1", good(_lib, item_offset=2 ** 32 - 81), {}),
             ("item_offset = 2^32", good(_lib, item_offset=2 ** 32), dict(B=1)),
             ("B * 41 > 2^32", good(_lib), dict(B=2 ** 32 // 41 + 1)),
             ("table off by 4", good(_lib), dict(table=ok + 4)),
             ("x_out off by 8", good(_lib), dict(out=ok + 8)),
             ("plain argument: B = 0", good(_lib), dict(B=0))]
    for field in ("gain_sigma", "amp_sigma", "noise_sigma"):
        for name, v in (("negative", -0.1), ("above 2", 2.5), ("NaN", nan), ("inf", inf)):
            cases.append((f"{field} {name}", good(_lib, **{field: v}), {}))
    for name, aug, kw in cases:
        rc = call(aug, **kw)
        msg = lib.cp_last_error()
        assert rc == 10001, (name, rc, msg)
        assert b"cp_gather_groups_aug" in msg, (name, msg)
    # the last item a call may hold is item 2^32 - 1: the limit itself is not refused by the host checks ... but nothing may be
    # enqueued from here, so the accepted side is covered on the device (tests/test_gpu_augment.py, item_offset = 2^31 + 5)


def test_augment_validation_errors():
    from contrastiveprosthetics_amd.augment import Augment, salt_of
    nan, inf = float("nan"), float("inf")
    bad = [dict(shift=8), dict(shift=-8), dict(shift=(2, 1)), dict(shift=(-8, 0)), dict(shift=(0, 8)), dict(shift=(1, 2, 3)),
           dict(shift="ab"), dict(p_drop=-0.1), dict(p_drop=1.1), dict(p_drop=nan), dict(dead=(12,)), dict(dead=(-1,)),
           dict(fill=inf), dict(fill=nan), dict(mean_std=np.ones(23)), dict(mean_std=np.zeros(24)),
           dict(mean_std=np.full(24, nan)), dict(seed=-1), dict(seed=2 ** 32)]
    for f in ("gain_sigma", "amp_sigma", "noise_sigma"):
        bad += [{f: -0.1}, {f: 2.01}, {f: nan}, {f: inf}]
    for kw in bad:
        with pytest.raises(ValueError):
            Augment(**kw)
    a = Augment()
    assert not a.active and a.count == 0 and a.shift == (0, 0)
    assert Augment(shift=2).shift == (2, 2) and Augment(shift=2).active and Augment(shift=(-7, 7)).active
    for kw in (dict(p_drop=0.1), dict(dead=(3,)), dict(gain_sigma=0.1), dict(amp_sigma=0.1), dict(noise_sigma=0.1)):
        assert Augment(**kw).active, kw
    assert not Augment(fill=1.0, mean_std=np.ones(24), seed=5).active          # nothing to fill, nothing to renormalise
    b = Augment(dead=(11, 0, 0), seed=9)
    assert b.dead == (0, 11) and b.dead_mask == 0x801 and b.config()["seed"] == 9 and b.config()["dead"] == (0, 11)
    assert [b.next_salt(), b.next_salt()] == [0x9E3779B1, (2 * 0x9E3779B1) & 0xFFFFFFFF] and b.count == 2
    assert salt_of(3) == (3 * 0x9E3779B1) & 0xFFFFFFFF
    s = b.struct(7, item_offset=2 ** 31 + 5, state_addr=0x7F1234567890)
    assert (s.salt, s.item_offset, s.dead_mask, s.salt_state_lo, s.salt_state_hi) == (7, 2 ** 31 + 5, 0x801, 0x34567890, 0x7F12)


def test_hash_and_normal_constant():
    from contrastiveprosthetics_amd import augment as A

    def h(x):                                                     # hash32 of csrc/common.cuh in Python integers
        x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
        return x
    xs = [0, 1, 0xFFFFFFFF, 0x9E3779B9, 123456789]
    assert [int(v) for v in A.hash32(np.array(xs, dtype=np.uint64))] == [h(x) for x in xs]
    src = open(os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc", "kernels_misc.cuh")).read()
    lit = re.search(r"#define AUG_NORM_C (0x[0-9a-fp.\-]+)f", src).group(1)
    assert float.fromhex(lit) == float(A.NORM_C) == float(np.float32(1.0 / np.sqrt((65536.0 ** 2 - 1) / 3)))
    assert 131070 * float(A.NORM_C) < 3.47
    # the chain by hand for one (seed, salt, item): k0 = h(seed ^ h(salt + c)), k = h(k0 + i), word(j) = h(k ^ (j a + b))
    seed, salt, i = 77, 0xDEADBEEF, 2 ** 31 + 9
    k = h((h(seed ^ h((salt + 0x9E3779B9) & 0xFFFFFFFF)) + i) & 0xFFFFFFFF)
    word = lambda j: h(k ^ ((j * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF))
    a = A.Augment(shift=(-3, 3), p_drop=0.25, gain_sigma=0.3, amp_sigma=0.2, noise_sigma=0.1, seed=seed)
    d = a.draws(i, 1, 3, salt)
    assert d["shift"][0] == -3 + ((word(0) * 7) >> 32)
    halves = lambda j: [word(j) & 0xFFFF, word(j) >> 16]
    assert [bool(x) for x in d["dead"][0]] == [halves(1 + c // 2)[c & 1] < 16384 for c in range(12)]
    n = lambda j: np.float32(sum(halves(j) + halves(j + 1)) - 131070) * A.NORM_C
    assert d["n_gain"][0, 5] == n(8 + 10) and d["n_amp"][0] == n(32) and d["n_noise"][0, 2, 7] == n(34 + 2 * (24 + 7))


def test_draw_statistics_of_the_reference():
    """2,624 items x 12 channels, three (seed, salt) pairs.  Bounds are 5 sigma of the estimator under the ideal law (derived,
    not measured): a frequency of probability p over n draws has sigma sqrt(p (1 - p) / n); the mean of m unit normals
    1 / sqrt(m); their standard deviation sqrt((kurtosis - 1) / (4 m)) with the Irwin-Hall(4) kurtosis 3 - 1.2 / 4 = 2.7."""
    from contrastiveprosthetics_amd.augment import Augment, salt_of
    n = 2624
    shifts = []
    for seed, salt in ((0, salt_of(1)), (1, salt_of(2)), (12345, salt_of(3))):
        a = Augment(shift=(-3, 3), p_drop=0.25, gain_sigma=0.3, amp_sigma=0.2, noise_sigma=0.1, seed=seed)
        d = a.draws(0, n, 1, salt)
        freq = np.bincount(d["shift"] + 3, minlength=7) / n
        assert d["shift"].min() >= -3 and d["shift"].max() <= 3
        assert np.abs(freq - 1 / 7).max() <= 5 * np.sqrt((1 / 7) * (6 / 7) / n), freq
        m = n * 12
        assert abs(d["dead"].mean() - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / m)
        for name, cnt in (("n_gain", m), ("n_noise", m), ("n_amp", n)):
            x = d[name].astype(np.float64).reshape(-1)
            assert x.size == cnt and np.abs(x).max() < 3.47
            assert abs(x.mean()) <= 5 / np.sqrt(cnt), (name, x.mean())
            assert abs(x.std() - 1) <= 5 * np.sqrt(1.7 / (4 * cnt)), (name, x.std())
        shifts.append(d["shift"])
        # the draws of an item depend on (seed, salt, item) alone: a window of the same stream drawn on its own is the same
        sub = a.draws(1000, 50, 1, salt)
        assert all(np.array_equal(sub[k], d[k][1000:1050]) for k in sub)
    assert not any(np.array_equal(shifts[i], shifts[j]) for i in range(3) for j in range(i))
    # three salts of ONE seed: no two give the same shift vector
    a = Augment(shift=(-3, 3), seed=4)
    vs = [a.draws(0, n, 1, salt_of(k))["shift"] for k in (1, 2, 3)]
    assert not any(np.array_equal(vs[i], vs[j]) for i in range(3) for j in range(i))


def test_reference_composes_as_documented():
    from contrastiveprosthetics_amd.augment import Augment
    from contrastiveprosthetics_amd.online import rotations
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 12)).astype(np.float32)
    assert np.array_equal(Augment().reference(x, 0, 25, 1), x.astype(np.float64))
    for s in (-7, -1, 1, 3):
        assert np.array_equal(Augment(shift=s).reference(x, 3, 1, 9), x.astype(np.float64)[:, rotations()[s % 8]])
    ms = np.concatenate([np.linspace(5, 60, 12), np.linspace(1, 9, 12)]).astype(np.float32)
    y, p = Augment(shift=2, dead=(0, 11), fill=-1.5, mean_std=ms).reference(x, 0, 25, 1, parts=True)
    assert np.all(y[:, [0, 11]] == -1.5) and np.array_equal(y[:, 8:11], x[:, 8:11].astype(np.float64))     # c == d, G == 1: x itself
    c = p["c"][0]
    m, sd = ms[:12].astype(np.float64), ms[12:].astype(np.float64)
    want = ((x[:, c].astype(np.float64) * sd[c] + m[c]) - m) / sd
    assert np.array_equal(y[:, 1:8], want[:, 1:8])
    # the V rows of an item share shift, gain and dead set; noise differs per row
    a = Augment(shift=(-3, 3), p_drop=0.3, gain_sigma=0.3, noise_sigma=0.1, seed=2)
    _, p = a.reference(np.ones((75, 12), np.float32), 10, 25, 5, parts=True)
    for it in range(3):
        blk = slice(25 * it, 25 * it + 25)
        assert len(set(p["shift"][blk])) == 1 and (p["G"][blk] == p["G"][blk][0]).all() and (p["dead"][blk] == p["dead"][blk][0]).all()
        assert len(np.unique(p["noise"][blk][:, 0])) == 25
