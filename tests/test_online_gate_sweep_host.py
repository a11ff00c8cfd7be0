"""CPU checks of the gate sweep (contrastiveprosthetics_amd/online.py sweep_gate, csrc/online_gate.cuh og_sweep_kernel): the score
on sequences worked out by hand, `expected_commands` against a brute-force loop, `pick_gate`'s filter and tie order, the two C
entries' declarations, sizes and refusals before any device call, and the wrapper's refusals through a stubbed device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
SWEEP = ["cp_online_gate_sweep_scratch_bytes", "cp_online_gate_sweep"]
ERR_ARG = 10001
KEYS = ("n_cue", "n_rest", "hit", "wrong", "false_active", "switches", "segments", "reached", "latency_sum", "wrong_segments")


# ---------------------------------------------------------------------------------------------------------------------------
# score_commands
# ---------------------------------------------------------------------------------------------------------------------------
def _score(command, expected):
    from contrastiveprosthetics_amd.online import score_commands
    out = score_commands(np.array(command, dtype=np.int32), np.array(expected, dtype=np.int64))
    assert tuple(out) == KEYS and all(type(v) is int for v in out.values())
    return out


def test_score_of_a_cue_with_a_late_hit_a_wrong_grasp_and_a_release():
    #           0   1   2   3   4   5   6   7   8   9
    expected = [-1, -1, 3, 3, 3, 3, 3, 3, -1, -1]           # rest, six windows of class 3, rest
    command = [-1, -1, -1, 5, 5, 3, 3, 3, 3, -1]            # a wrong grasp first, the hit at 5, released one window late
    assert _score(command, expected) == dict(
        n_cue=6, n_rest=4, hit=3, wrong=2, false_active=1,   # hits 5, 6, 7; wrong 3, 4; still active at 8
        switches=3,                                          # at 3 (none -> 5), 5 (5 -> 3) and 9 (3 -> none)
        segments=1, reached=1, latency_sum=3,                # the segment starts at 2, its first hit is at 5
        wrong_segments=1)


def test_score_of_rest_with_a_false_activation():
    expected = [-1] * 6
    command = [-1, 2, 2, -1, -1, 4]
    assert _score(command, expected) == dict(n_cue=0, n_rest=6, hit=0, wrong=0, false_active=3, switches=3, segments=0, reached=0,
                                             latency_sum=0, wrong_segments=0)


def test_score_counts_two_segments_of_one_class_across_an_ignored_window():
    expected = [7, 7, -2, 7, 7, 7]                           # IGNORE at 2 ends the first segment
    command = [7, 7, 7, -1, -1, 7]                           # a hit at once; the second segment is reached at 5, two late
    assert _score(command, expected) == dict(n_cue=5, n_rest=0, hit=3, wrong=0, false_active=0,
                                             switches=3,     # at 0 (command[-1] is none), 3 and 5; 2 is ignored but walked
                                             segments=2, reached=2, latency_sum=2, wrong_segments=0)
    # neighbours of different classes are two segments too; the second is never reached and wrong throughout
    assert _score([1, 1, 1, 1], [1, 1, 2, 2]) == dict(n_cue=4, n_rest=0, hit=2, wrong=2, false_active=0, switches=1, segments=2,
                                                     reached=1, latency_sum=0, wrong_segments=1)


def test_score_of_the_empty_sequence():
    assert _score([], []) == dict.fromkeys(KEYS, 0)
    from contrastiveprosthetics_amd.online import score_commands
    with pytest.raises(ValueError):
        score_commands(np.zeros(3, int), np.zeros(4, int))


def test_score_against_a_window_by_window_loop():
    """the vectorised definition against the sentence-by-sentence loop, on random sequences"""
    from contrastiveprosthetics_amd.online import score_commands
    rng = np.random.default_rng(4)
    for _ in range(30):
        n = int(rng.integers(1, 200))
        exp = np.repeat(rng.choice([-2, -1, 0, 3, 9], n), rng.integers(1, 6, n))[:n]
        cmd = np.repeat(rng.choice([-1, 0, 3, 9], n), rng.integers(1, 4, n))[:n]
        want = dict.fromkeys(KEYS, 0)
        prev, seg, start, got_hit, got_wrong = -1, None, 0, False, False
        for j in range(n):
            e, c = int(exp[j]), int(cmd[j])
            want["switches"] += c != prev
            prev = c
            if e >= 0:
                if seg != e:
                    seg, start, got_hit, got_wrong = e, j, False, False
                    want["segments"] += 1
                want["n_cue"] += 1
                if c == e:
                    want["hit"] += 1
                    if not got_hit:
                        got_hit = True
                        want["reached"] += 1
                        want["latency_sum"] += j - start
                elif c >= 0:
                    want["wrong"] += 1
                    want["wrong_segments"] += not got_wrong
                    got_wrong = True
            else:
                seg = None
                if e == -1:
                    want["n_rest"] += 1
                    want["false_active"] += c != -1
        assert score_commands(cmd, exp) == want


# ---------------------------------------------------------------------------------------------------------------------------
# expected_commands
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 7])
@pytest.mark.parametrize("rest", [None, 0])
def test_expected_commands_against_a_brute_force_loop(phase, rest):
    from contrastiveprosthetics_amd.online import IGNORE, REST, expected_commands, windows_before
    assert (REST, IGNORE) == (-1, -2)
    rng = np.random.default_rng(5)
    ids = [2, 5, 11]
    # stretches of one label: classes, rest (0), a label that is no column (8), unlabelled (-1); edges make mixed windows
    labels = np.repeat(rng.choice([0, 2, 5, 11, 8, -1], 60), rng.integers(5, 90, 60))
    got = expected_commands(labels, ids, phase=phase, rest=rest)
    n = windows_before(labels.shape[0], phase)
    assert got.shape == (n,) and got.dtype == np.int64
    want, kinds = [], set()
    for k in range(n):
        span = labels[phase + 20 * k:phase + 20 * k + 11]
        assert span.shape == (11,)
        if len(set(span.tolist())) > 1:
            want.append(IGNORE)
            kinds.add("mixed")
        elif span[0] < 0:
            want.append(IGNORE)
            kinds.add("unlabelled")
        elif rest is not None and span[0] == rest:
            want.append(REST)
            kinds.add("rest")
        elif int(span[0]) in ids:
            want.append(int(span[0]))
            kinds.add("class")
        else:
            want.append(IGNORE)
            kinds.add("other")
    assert kinds == {"mixed", "unlabelled", "class", "other"} | ({"rest"} if rest is not None else set())
    assert got.tolist() == want
    if rest is None:
        assert REST not in got                                           # label 0 is then just a label that is no column


def test_expected_commands_refuses_bad_ids():
    from contrastiveprosthetics_amd.online import expected_commands
    lab = np.zeros(100, dtype=np.int64)
    for ids in ([], [3, 2], [2, 2], [-1, 4], list(range(65))):
        with pytest.raises(ValueError):
            expected_commands(lab, ids)
    assert expected_commands(lab[:5], [0]).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------------
# pick_gate
# ---------------------------------------------------------------------------------------------------------------------------
def _scores(rows):
    """rows: one dict per config; missing keys are 0"""
    return {k: np.array([r.get(k, 0) for r in rows], dtype=np.int64) for k in KEYS}


def test_pick_gate_filters_then_orders_by_hit_latency_index():
    from contrastiveprosthetics_amd.online import pick_gate
    base = dict(n_cue=100, n_rest=100, reached=4)
    rows = [dict(base, hit=90, false_active=3),                          # 0: too many false activations (3 % > 2 %)
            dict(base, hit=95, wrong=6),                                 # 1: too many wrong grasps (6 % > 5 %)
            dict(base, hit=70, false_active=2, wrong=5, latency_sum=40), # 2: eligible, exactly at both limits
            dict(base, hit=80, latency_sum=40),                          # 3: eligible, more hits
            dict(base, hit=80, latency_sum=20),                          # 4: as many hits, reached sooner
            dict(base, hit=80, latency_sum=10, reached=2),               # 5: mean latency 5, the same as 4: the index decides
            dict(base, hit=80, latency_sum=24)]                          # 6: mean latency 6
    sc = _scores(rows)
    assert pick_gate(sc) == 4
    assert pick_gate(sc, max_false_rate=0.03) == 0                       # the limits are the caller's
    assert pick_gate(sc, max_wrong_rate=0.06) == 1
    assert pick_gate(_scores(rows[:3])) == 2
    assert pick_gate(_scores(rows[:2])) is None
    assert pick_gate(_scores(rows[3:4] * 3)) == 0                        # all the same: the smallest index
    assert isinstance(pick_gate(sc), int)


def test_pick_gate_takes_a_rate_over_nothing_as_zero():
    from contrastiveprosthetics_amd.online import pick_gate
    # no rest windows and no cue windows at all: both rates are 0, reached 0 -> latency_sum / max(reached, 1)
    assert pick_gate(_scores([dict(), dict()])) == 0
    # no rest windows: false_active cannot exclude; no reached segment: latency 0 / 1
    rows = [dict(n_cue=10, hit=0, wrong=1), dict(n_cue=10, hit=3, wrong=0, reached=1, latency_sum=9), dict(n_cue=10, hit=3)]
    assert pick_gate(_scores(rows)) == 2                                 # hit 3 twice; latency 0 beats 9
    assert pick_gate(_scores(rows[:1])) is None                          # 10 % wrong
    assert pick_gate(_scores([dict(n_rest=10, false_active=1)])) is None
    assert pick_gate(_scores([dict(n_rest=10, false_active=1)]), max_false_rate=0.1) == 0


def test_gate_grid_is_the_cartesian_product():
    from contrastiveprosthetics_amd.online import gate_grid
    grid = gate_grid(dwell=[1, 3], release=[0, 5, 9], weight=["margin"])
    assert len(grid) == 6 and grid[0] == dict(dwell=1, release=0, weight="margin") and grid[1]["release"] == 5
    assert grid[3] == dict(dwell=3, release=0, weight="margin")
    assert gate_grid() == [{}]
    with pytest.raises(ValueError, match="dwel"):
        gate_grid(dwel=[1])


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_sweep_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import score_commands
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in SWEEP:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    n_scores = int(re.search(r"#define\s+CP_ONLINE_GATE_SCORES\s+(\d+)", hdr).group(1))
    assert n_scores == _lib.CP_ONLINE_GATE_SCORES == len(score_commands(np.zeros(0, int), np.zeros(0, int))) == 10
    n_max = int(re.search(r"#define\s+CP_ONLINE_GATE_SWEEP_MAX_CONFIGS\s+(\d+)", hdr).group(1))
    assert n_max == _lib.CP_ONLINE_GATE_SWEEP_MAX_CONFIGS == 65536
    assert lib.cp_version() == 112


def test_sweep_scratch_is_twelve_bytes_per_row(lib):
    f = lib.cp_online_gate_sweep_scratch_bytes
    for n in (1, 63, 64, 65, 6000, 60000, 10 ** 7):
        assert 12 * n <= f(n) < 12 * n + 256 and f(n) % 256 == 0, n
    assert f(64 * 1000 + 64) - f(64 * 1000) == 12 * 64               # (64 rows are a multiple of the alignment)
    assert f(0) == f(1)


def test_sweep_refuses_bad_arguments_before_any_device_call(lib):
    """host memory in every pointer: each refusal returns before a launch, which on this machine would fail differently"""
    M, K, G = 10, 5, 3
    lg = (ctypes.c_float * (M * 8))()
    exp = (ctypes.c_int32 * M)()
    cfg = (ctypes.c_int32 * (6 * G))()
    thr = (ctypes.c_float * (64 * G))()
    scores = (ctypes.c_int64 * (10 * G))()
    cmds = (ctypes.c_int32 * (G * M))()
    need = lib.cp_online_gate_sweep_scratch_bytes(M)
    buf = ctypes.create_string_buffer(need + 256)
    scratch = (ctypes.addressof(buf) + 255) // 256 * 256
    good = dict(logits=lg, ldl=8, n_rows=M, n_classes=K, expected=exp, configs=cfg, min_cosine=thr, n_configs=G, scratch=scratch,
                scratch_bytes=need, scores=scores, commands=cmds)

    def refused(what, **kw):
        a = dict(good, **kw)
        rc = lib.cp_online_gate_sweep(a["logits"], a["ldl"], a["n_rows"], a["n_classes"], a["expected"], a["configs"], a["min_cosine"],
                                      a["n_configs"], a["scratch"], a["scratch_bytes"], a["scores"], a["commands"], None)
        assert rc == ERR_ARG, (kw, rc)
        msg = lib.cp_last_error()
        assert b"cp_online_gate_sweep" in msg and what.encode() in msg, (kw, msg)

    refused("n_classes", n_classes=0)
    refused("n_classes", n_classes=65)
    refused("ldl", n_classes=9)                                          # more classes than the rows are long
    refused("ldl", ldl=4)
    refused("n_configs", n_configs=0)
    refused("n_configs", n_configs=65537)
    refused("n_rows", n_rows=0)
    refused("n_rows", n_rows=-5)
    refused("scratch", scratch_bytes=12 * M - 1)
    refused("scratch", scratch_bytes=0)
    refused("scratch", scratch=None)
    refused("logits", logits=None)
    refused("expected_slot", expected=None)
    refused("configs", configs=None)
    refused("min_cosine", min_cosine=None)
    refused("scores", scores=None)
    refused("misaligned", scores=ctypes.addressof(scores) + 4)
    refused("misaligned", commands=ctypes.addressof(cmds) + 2)


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper: what it refuses before the device is asked for anything
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from contrastiveprosthetics_amd import online
    calls = []

    def stub(logits, slots, k, cfg, thr, want_commands):
        calls.append((slots.copy(), k, cfg.copy(), thr.copy(), want_commands))
        import torch
        return np.zeros((cfg.shape[0], 10), dtype=np.int64), (torch.zeros(cfg.shape[0], logits.shape[0], dtype=torch.int32)
                                                              if want_commands else None)

    monkeypatch.setattr(online, "_sweep_dev", stub)
    return calls


def test_sweep_gate_refuses_bad_configs_without_a_device_call(no_device):
    import torch
    from contrastiveprosthetics_amd.online import sweep_gate
    ids = [1, 4, 6]
    lg = torch.zeros(4, 3)
    exp = np.array([-1, 4, 4, -2])
    bad = [([dict(dwel=2)], "dwel"),                                     # an unknown key
           ([dict(dwell=0)], "dwell must be an int >= 1"),               # CommandGate's own messages
           ([dict(weight="x")], "weight must be 'count' or 'margin'"),
           ([dict(min_cosine={5: 0.5})], "class id 5"),                  # a threshold for an id that is no column
           ([{}] * 65537, "65536"),
           ([], "65536"),
           ([dict(release=-1)], "release must be an int >= 0"),
           ([dict(min_votes=0)], "min_votes"),
           ([dict(vote=257)], "vote must lie in 1..256"),
           ([dict(vote=0)], "vote"),
           ([dict(min_margin=float("nan"))], "min_margin must be finite"),
           ([dict(min_cosine=float("nan"))], "min_cosine must not be NaN"),
           ([dict(dwell=1.5)], "dwell"),
           ([dict(dwell=2), dict(dwell=True)], "dwell")]                 # the second of two
    for configs, what in bad:
        with pytest.raises(ValueError, match=re.escape(what)):
            sweep_gate(lg, exp, ids, configs)
    with pytest.raises(ValueError, match="expected"):
        sweep_gate(lg, exp[:3], ids, [{}])
    with pytest.raises(ValueError, match="expected"):
        sweep_gate(lg, np.array([0, 1, 4, 6]), ids, [{}])               # 0 is no class id here
    with pytest.raises(ValueError, match="logits"):
        sweep_gate(torch.zeros(4, 2), exp, ids, [{}])
    with pytest.raises(ValueError, match="ids"):
        sweep_gate(lg, exp, [4, 1, 6], [{}])
    with pytest.raises(ValueError, match="GPU"):
        sweep_gate(lg, exp, ids, [{}])                                   # valid, but host logits: refused before the device
    assert no_device == []


def test_sweep_gate_hands_the_device_slots_configs_and_thresholds(no_device, monkeypatch):
    import torch
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import sweep_gate

    class OnDevice(torch.Tensor):                                        # host memory that says it is on the GPU
        @property
        def device(self):
            return torch.device("cuda:0")

    ids = [1, 4, 6]
    lg = torch.zeros(4, 3).as_subclass(OnDevice)
    configs = [{}, dict(min_cosine={4: 0.5}, default=0.25, min_margin=0.125, min_votes=3, dwell=4, release=0, weight="margin", vote=9)]
    out, cmds = sweep_gate(lg, np.array([-1, 4, 6, -2]), ids, configs, return_commands=True)
    assert tuple(out) == KEYS and all(v.shape == (2,) and v.dtype == np.int64 for v in out.values())
    assert cmds.shape == (2, 4) and (cmds == 1).all()                    # the stub's slot 0 everywhere: class id 1
    (slots, k, cfg, thr, want), = no_device
    assert slots.tolist() == [-1, 1, 2, -2] and slots.dtype == np.int32 and k == 3 and want
    assert cfg.dtype == np.int32 and cfg.shape == (2, 6) and cfg.nbytes == 2 * ctypes.sizeof(_lib.cp_online_gate_config)
    c = _lib.cp_online_gate_config.from_buffer_copy(cfg[1].tobytes())
    assert (c.vote, c.min_votes, c.dwell, c.release, c.weight, c.min_margin) == (9, 3, 4, 0, 1, 0.125)
    c = _lib.cp_online_gate_config.from_buffer_copy(cfg[0].tobytes())    # CommandGate's defaults
    assert (c.vote, c.min_votes, c.dwell, c.release, c.weight, c.min_margin) == (25, 1, 1, 1, 0, 0.0)
    assert thr.shape == (2, 64) and thr[0, :3].tolist() == [-2.0] * 3 and thr[1, :3].tolist() == [0.25, 0.5, 0.25]


def test_command_gate_use_applies_a_config():
    from test_online_gate_host import StubDecoder
    from contrastiveprosthetics_amd.online import CommandGate
    g = CommandGate(StubDecoder(), dwell=4)
    g._ids_seen[0] = object()
    g.use(dict(dwell=2, release=0, min_margin=0.25, weight="margin", min_votes=3, min_cosine={4: 0.5}, default=0.125, vote=25))
    assert (g._cfg.dwell, g._cfg.release, g._cfg.min_margin, g._cfg.weight, g._cfg.min_votes) == (2, 0, 0.25, 1, 3)
    assert g._thr[0] == ({4: 0.5}, 0.125) and g._ids_seen[0] is None      # the thresholds go in with the next launch
    g.use(dict(dwell=5))                                                 # the other settings and the thresholds stay
    assert (g._cfg.dwell, g._cfg.release) == (5, 0) and g._thr[0] == ({4: 0.5}, 0.125)
    for bad in (dict(vote=7), dict(dwel=1), dict(dwell=0, min_cosine=0.5), dict(min_cosine=float("nan"), dwell=9)):
        with pytest.raises(ValueError):
            g.use(bad)
    assert g._cfg.dwell == 5 and g._thr[0] == ({4: 0.5}, 0.125)           # a refused config changes nothing


def test_sweep_names_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    from contrastiveprosthetics_amd import online
    for n in ("REST", "IGNORE", "expected_commands", "score_commands", "pick_gate", "sweep_gate", "gate_grid"):
        assert getattr(pkg, n) is getattr(online, n), n
