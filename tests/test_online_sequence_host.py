"""CPU checks of the grasp sequence decoder (contrastiveprosthetics_amd/sequence.py, csrc/online_sequence.cuh): the numpy
definition against brute force over all paths and against its own identities, the matrix builders on examples worked out by
hand, what the Python side refuses, and the C entries' refusals before any launch.  Every comparison is exact."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG = 10001                          # CP_ERR_ARG
F = np.float32
ONE = 1 << 20
SEQ = ("cp_online_seq_workspace_bytes", "cp_online_seq_set_model", "cp_online_seq_reset", "cp_online_seq_push",
       "cp_online_seq_sweep_scratch_bytes", "cp_online_seq_sweep")


def random_case(rng, K, M, dense=True):
    lg = rng.uniform(-1.0, 1.0, (M, K)).astype(F)
    C = rng.integers(0, 3 * ONE + 1, (K + 1, K + 1)).astype(np.int32) if dense else np.zeros((K + 1, K + 1), dtype=np.int32)
    thr = rng.uniform(-0.5, 0.5, K).astype(F)
    return lg, C, thr


# ---------------------------------------------------------------------------------------------------------------------------
# the definition is Viterbi
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_pointers_hold_a_maximum_score_path_by_brute_force():
    """K in 1..3, M in 1..6: the path read back from the pointers at lag 0 scores what the best of all (K+1)^M paths scores
    (scores are compared, not paths: ties exist).  A path's score: the start is free (every score is 0 before the first window),
    then minus C along the path plus the emission of every state on it."""
    from contrastiveprosthetics_amd.sequence import SequenceReference, quantise
    rng = np.random.default_rng(5)
    seen = set()
    for case in range(200):
        K, M = int(rng.integers(1, 4)), int(rng.integers(1, 7))
        seen.add((K, M))
        lg, C, thr = random_case(rng, K, M)
        ref = SequenceReference(np.arange(K), thr, C, 0)
        ref.run_rows(lg)
        s = int(np.argmax(ref.score))
        path = [s]
        for t in range(M - 1, 0, -1):
            s = int(ref.ring[t][s])
            path.append(s)
        path = path[::-1]
        e = np.zeros((M, K + 1), dtype=np.int64)
        e[:, :K] = quantise(lg).astype(np.int64) - quantise(thr)

        def score(p):
            v = -int(C[:, p[0]].min()) + int(e[0, p[0]])
            for t in range(1, M):
                v += int(e[t, p[t]]) - int(C[p[t - 1], p[t]])
            return v

        best = max(score(p) for p in itertools.product(range(K + 1), repeat=M))
        assert score(path) == best, (case, K, M)
    assert len(seen) == 18                                             # every K with every M


# ---------------------------------------------------------------------------------------------------------------------------
# properties of the reference
# ---------------------------------------------------------------------------------------------------------------------------
def run_cut(ref, lg, cuts):
    out = [ref.run_rows(lg[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return [np.concatenate([o[i] for o in out]) for i in range(3)]


@pytest.mark.parametrize("lag", [0, 1, 7, 63])
def test_the_reference_does_not_depend_on_the_cut(lag):
    from contrastiveprosthetics_amd.sequence import SequenceReference
    rng = np.random.default_rng(lag)
    K, M = 5, 150
    lg, C, thr = random_case(rng, K, M)
    C //= 8
    ids = np.array([2, 3, 11, 40, 41])
    whole = SequenceReference(ids, thr, C, lag)
    want = whole.run_rows(lg)
    assert len({int(c) for c in want[0]}) >= 3
    for cuts in ([0, 1, 2, 3, 80, M], [0, 64, 128, M], sorted({0, M, *rng.integers(0, M, 9).tolist()})):
        ref = SequenceReference(ids, thr, C, lag)
        got = run_cut(ref, lg, cuts)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), cuts
        assert np.array_equal(ref.score, whole.score) and ref.n == whole.n == M
        assert len(ref.ring) == 64 and all(np.array_equal(a, b) for a, b in zip(ref.ring, whole.ring))


def test_without_costs_now_is_the_first_maximum_and_command_is_now_delayed():
    from contrastiveprosthetics_amd.sequence import SequenceReference, quantise
    rng = np.random.default_rng(3)
    K, M = 6, 120
    lg, C, _ = random_case(rng, K, M, dense=False)
    lg[10] = lg[10, 0]                                                 # a row of equal logits: the first slot wins
    lg[11, 3] = lg[11, 1] = 1.5                                        # two equal maxima: slot 1
    ids = np.arange(10, 10 + K)
    now0 = SequenceReference(ids, -2.0, C, 0).run_rows(lg)[1]
    assert np.array_equal(now0, ids[quantise(lg).argmax(axis=1)]) and now0[10] == ids[0] and now0[11] == ids[1]
    for lag in (0, 1, 25, 63):
        cmd, now, _ = SequenceReference(ids, -2.0, C, lag).run_rows(lg)
        assert np.array_equal(now, now0)
        assert (cmd[:lag] == -1).all() and np.array_equal(cmd[lag:], now0[:M - lag]), lag


def floor_rows(K=3, quiet=200, rise=40):
    """200 rows of logits -5.0, then class 1 rising from -1 to 1"""
    lg = np.full((quiet + rise, K), -5.0, dtype=F)
    lg[quiet:, 1] = np.linspace(-1.0, 1.0, rise, dtype=F)
    return lg


def test_the_lowest_score_is_reached_and_held():
    """200 rows of logits -5.0 under min_cosine 2.0, then a class rising.  Every class loses q(-5) - q(2) = -2^22 per window
    against none.  With entering a class as good as forbidden (2^28) a class score falls by 2^22 per window until coming back
    from none is the better predecessor: it then stays at exactly -2^28 - 2^22, window after window, and follows the emission
    when the class rises (-2^28 + e).
    The clamp at FLOOR = -2^29 itself cannot be reached through the interface: costs are at most 2^28 and the best state
    has score 0, so best[j] >= -2^28, new[j] >= -2^28 - 2^22 and, the maximum of new being at most 2^22, every score is at least
    -2^28 - 2^23 > -2^29.  FLOOR is a guard for a workspace the stage did not write; what is asserted is the bound above."""
    from contrastiveprosthetics_amd.sequence import FLOOR, SequenceReference, potts, quantise
    assert FLOOR == -(1 << 29)
    lowest = -(1 << 28) - (1 << 22)
    assert FLOOR < -(1 << 28) - (1 << 23) < lowest
    lg = floor_rows()
    C = potts(3, 0.5, 300.0, 0.5, through_rest=True)
    assert C[3, 0] == C[0, 1] == 1 << 28
    ref = SequenceReference([4, 5, 9], 2.0, C, 0)
    cmd, now, lead = ref.run_rows(lg[:65])
    assert ref.score.tolist() == [-65 << 22, -65 << 22, -65 << 22, 0]    # still falling: 65 * 2^22 = 2^28 + 2^22, reached
    ref.run_rows(lg[65:100])
    assert ref.score.tolist() == [lowest] * 3 + [0]
    cmd, now, lead = ref.run_rows(lg[100:200])
    assert ref.score.tolist() == [lowest] * 3 + [0]                        # held
    assert (cmd == -1).all() and (now == -1).all() and (lead == -lowest).all()
    for t in range(200, 240):
        ref.run_rows(lg[t:t + 1])
        e = int(quantise(lg[t, 1])) - (1 << 21)
        assert ref.score.tolist() == [lowest, -(1 << 28) + e, lowest, 0], t
    assert ref.score.min() > FLOOR


def test_a_non_finite_row_carries_no_evidence():
    from contrastiveprosthetics_amd.sequence import FLOOR, SequenceReference, potts
    rng = np.random.default_rng(8)
    K = 4
    lg = rng.uniform(-0.3, 0.6, (30, K)).astype(F)
    C = potts(K, 0.25, 0.25, 0.25)
    for bad in (np.nan, np.inf, -np.inf):
        a, b = SequenceReference(np.arange(K), 0.1, C, 0), SequenceReference(np.arange(K), 0.1, C, 0)
        a.run_rows(lg)
        b.run_rows(lg)
        before = a.score.astype(np.int64)
        row = lg[7].copy()
        row[2] = bad
        a.step(row)
        b.step(lg[7])
        assert a.n == b.n == 31 and len(a.ring) == 31
        # e = 0 everywhere: the step of the bad row is the transition alone, from the scores before it
        want = (before[:, None] - C).max(axis=0)
        assert np.array_equal(a.score, np.maximum(want - want.max(), FLOOR)), bad
        assert not np.array_equal(a.score, b.score), bad               # and the finite row would have moved them otherwise


# ---------------------------------------------------------------------------------------------------------------------------
# potts, transitions_from_cues, sequence_grid
# ---------------------------------------------------------------------------------------------------------------------------
def test_potts_by_hand():
    from contrastiveprosthetics_amd.sequence import potts
    h, q, o = ONE // 2, ONE // 4, ONE
    assert potts(2, 0.5, 0.25, 1.0).tolist() == [[0, h, o], [h, 0, o], [q, q, 0]]
    big = 1 << 28
    assert potts(2, 0.5, 0.25, 1.0, through_rest=True).tolist() == [[0, big, o], [big, 0, o], [q, q, 0]]
    assert potts(1, 3.0, 0.0, 1e9).tolist() == [[0, big], [0, 0]]      # (no other class; a price past 256 is 2^28)
    assert potts(64, 0.5, 0.5, 0.5).shape == (65, 65) and potts(3, 0.3, 0.3, 0.3).dtype == np.int32
    assert potts(2, 2.5e-7, 0, 0)[0, 1] == 0 and potts(2, 1.5 / ONE, 0, 0)[0, 1] == 2          # half-even
    for bad in (dict(k=0), dict(k=65), dict(k=True), dict(k=2.0), dict(switch=-0.1), dict(engage=float("nan")),
                dict(release=float("inf"))):
        with pytest.raises(ValueError):
            potts(**{**dict(k=2, switch=0.5, engage=0.5, release=0.5), **bad})


def test_transitions_from_cues_by_hand():
    from contrastiveprosthetics_amd.online import IGNORE, REST
    from contrastiveprosthetics_amd.sequence import transitions_from_cues
    ids = [3, 7]
    #      3  3  3  R  R  7  7  I  3  R      pairs: 3>3 x2, 3>R, R>R, R>7, 7>7, (7>I, I>3 broken), 3>R
    exp = [3, 3, 3, REST, REST, 7, 7, IGNORE, 3, REST]
    counts = np.array([[2, 0, 2], [0, 1, 0], [0, 1, 1]], dtype=np.float64) + 1.0
    p = counts / counts.sum(axis=1, keepdims=True)
    want = np.rint(-np.log(p) * 0.25 * ONE).astype(np.int64)
    want -= want.min(axis=1, keepdims=True)
    got = transitions_from_cues(exp, ids, 0.25)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert got[0, 0] == 0 and got[0, 2] == 0 and got[0, 1] == int(np.rint(np.log(7) * 0.25 * ONE)) - int(np.rint(np.log(7 / 3) * 0.25 * ONE))
    # without a floor a transition never seen is as good as forbidden, and a state never left costs nothing
    bare = transitions_from_cues(exp, ids, 0.25, floor_count=0)
    assert bare[0, 1] == (1 << 28) - bare_min(exp, 0.25) and bare[1].tolist() == [1 << 28, 0, 1 << 28]
    assert transitions_from_cues([IGNORE, IGNORE], ids, 1.0, floor_count=0).tolist() == [[0] * 3] * 3
    for bad in (dict(scale=0.0), dict(scale=float("nan")), dict(floor_count=-1), dict(expected=[5]), dict(expected=[-3]),
                dict(ids=[7, 3]), dict(expected=[0.5])):
        with pytest.raises(ValueError):
            transitions_from_cues(**{**dict(expected=exp, ids=ids, scale=0.25), **bad})


def bare_min(exp, scale):
    """row 0 of the hand example without a floor: counts (2, 0, 2), so its minimum is rint(ln 2 * scale * 2^20)"""
    return int(np.rint(np.log(2.0) * scale * ONE))


def test_sequence_grid_and_config_refusals():
    from contrastiveprosthetics_amd.sequence import _sweep_configs, potts, sequence_grid
    a, b = dict(switch=0.5, engage=0.5, release=0.5), dict(switch=0.1, engage=0.2, release=0.3, through_rest=True)
    grid = sequence_grid(transitions=[a, b], lag=[0, 5], min_cosine=[0.1])
    assert grid == [dict(transitions=a, lag=0, min_cosine=0.1), dict(transitions=a, lag=5, min_cosine=0.1),
                    dict(transitions=b, lag=0, min_cosine=0.1), dict(transitions=b, lag=5, min_cosine=0.1)]
    with pytest.raises(ValueError):
        sequence_grid(dwell=[1])
    ids = np.array([3, 7, 8])
    same = potts(3, 0.5, 0.5, 0.5)
    costs, cfg, thr = _sweep_configs(grid + [dict(transitions=same, lag=63, min_cosine={7: 0.5}, default=0.25), {},
                                             dict(transitions=lambda i: potts(len(i), 0.1, 0.2, 0.3, True))], ids)
    assert costs.shape == (2, 4, 4) and costs.dtype == np.int32        # equal matrices are one model
    assert cfg.tolist() == [[0, 0], [0, 5], [1, 0], [1, 5], [0, 63], [0, 0], [1, 0]]
    assert thr.shape == (7, 64) and thr[4, :4].tolist() == [0.25, 0.5, 0.25, 0.0] and thr[5, :3].tolist() == [-2.0] * 3
    for bad in ([], [dict(lag=64)], [dict(lag=-1)], [dict(lag=1.0)], [dict(vote=3)], [dict(min_cosine=float("nan"))],
                [dict(min_cosine={4: 0.1})], [dict(default=0.1)], [dict(transitions=dict(switch=0.5))],
                [dict(transitions=dict(switch=-1, engage=0, release=0))], [dict(transitions=potts(2, 0.5, 0.5, 0.5))],
                [dict(transitions=np.full((4, 4), -1))], [dict(transitions=np.zeros((4, 4)))], [dict(transitions="potts")], [3]):
        with pytest.raises(ValueError):
            _sweep_configs(bad, ids)


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper, through a stub decoder: what it refuses before any launch
# ---------------------------------------------------------------------------------------------------------------------------
class StubDecoder:
    """what SequenceGate reads of a single-stream decoder"""

    def __init__(self, ids=(1, 4, 6)):
        import torch
        self.class_ids = torch.tensor(ids, dtype=torch.int32)
        self.n_seen, self.phase = 0, 0

    def push(self, raw, return_logits=False, return_windows=False):
        raise AssertionError("no push in a refusal")

    def reset(self):
        self.n_seen = 0


def test_sequence_gate_refusals_are_value_errors():
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.sequence import SequenceGate
    with pytest.raises(TypeError):
        SequenceGate(object())
    for bad in (dict(lag=64), dict(lag=-1), dict(lag=True), dict(min_cosine=float("nan")), dict(transitions=dict(switch=0.5)),
                dict(transitions=dict(switch=0.5, engage=0.5, release=0.5, dwell=1)), dict(transitions=3)):
        with pytest.raises(ValueError):
            SequenceGate(StubDecoder(), **bad)
    gate = SequenceGate(StubDecoder(), lag=3)
    st = gate.state()
    assert gate.lag == 3 and st["n"] == 0 and st["ring"] == [] and st["score"].size == 0 and gate.ws is None
    for bad in (dict(lag=99), dict(vote=2), dict(default=0.0), dict(min_cosine={1: float("nan")})):
        with pytest.raises(ValueError):
            gate.use(bad)
    assert gate.lag == 3
    gate.use(dict(lag=5, min_cosine={4: 0.3}, default=0.1, transitions=dict(switch=1, engage=1, release=1)))
    assert gate.lag == 5 and gate._thr[0] == ({4: 0.3}, 0.1)
    with pytest.raises(TypeError):
        gate.set_thresholds(0, 0.5)                                    # single-stream: no stream index
    with pytest.raises(TypeError):
        gate.push_packed(None, None)
    with pytest.raises(IndexError):
        gate.state(1)
    gate.decoder.n_seen = 40                                           # pushed behind the stage's back
    with pytest.raises(_lib.CpNativeError):
        gate.push(None)
    assert gate.ws is None                                             # nothing was allocated, nothing enqueued


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_sequence_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in SEQ:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    body = hdr[hdr.index("typedef struct cp_online_seq_config {"):hdr.index("} cp_online_seq_config;")]
    assert re.findall(r"\bint32_t\s+(\w+);", body) == [f[0] for f in _lib.cp_online_seq_config._fields_] == ["model", "lag"]
    assert ctypes.sizeof(_lib.cp_online_seq_config) == 8
    for name in ("CP_ONLINE_SEQ_RING", "CP_ONLINE_SEQ_MAX_COST", "CP_ONLINE_SEQ_FLOOR", "CP_ONLINE_SEQ_SWEEP_MAX_CONFIGS"):
        value = re.search(r"#define %s \(?(-?\d+)\)?" % name, text).group(1)
        assert int(value) == getattr(_lib, name), name
    assert int(re.search(r"#define CP_VERSION (\d+)", text).group(1)) == 112


def test_sequence_workspace_is_per_stream_state(lib):
    one = lib.cp_online_seq_workspace_bytes(1)
    # K, lag, n, head, ids[64], thr[64], the (65, 65) matrix, score[65] and 64 rows of 65 back-pointer bytes
    assert one >= 4 * (4 + 64 + 64 + 65 * 65 + 65) + 64 * 65 and one % 256 == 0
    sizes = [lib.cp_online_seq_workspace_bytes(s) for s in (1, 2, 64, 256)]
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3] <= 256 * one
    assert lib.cp_online_seq_workspace_bytes(0) == one
    assert lib.cp_online_seq_sweep_scratch_bytes(0) == 256 and lib.cp_online_seq_sweep_scratch_bytes(14514) == 14514 * 256


def test_sequence_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory as the 'workspace': every refusal returns before a launch, which without a GPU would fail differently"""
    from contrastiveprosthetics_amd import _lib
    S = 4
    need = lib.cp_online_seq_workspace_bytes(S)
    buf = ctypes.create_string_buffer(need + 256)
    ws = (ctypes.addressof(buf) + 255) // 256 * 256
    ids = (ctypes.c_int32 * 65)(*range(65))
    thr = (ctypes.c_float * 65)()
    cost = (ctypes.c_int32 * (65 * 65))()
    rows = (ctypes.c_int32 * S)()
    out = (ctypes.c_int32 * 8)()
    lg = (ctypes.c_float * 64)()
    sm, rs, pu, sw = "cp_online_seq_set_model", "cp_online_seq_reset", "cp_online_seq_push", "cp_online_seq_sweep"

    def err(rc, entry, what):
        assert rc == ERR_ARG, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    def each(what, n_streams=S, w=ws, nbytes=need):                  # every entry with a workspace refuses, one at a time
        err(lib.cp_online_seq_set_model(n_streams, w, nbytes, 0, ids, thr, 2, cost, 0, None), sm, what)
        err(lib.cp_online_seq_reset(n_streams, w, nbytes, -1, None), rs, what)
        err(lib.cp_online_seq_push(n_streams, w, nbytes, lg, 2, rows, rows, 1, out, out, out, None), pu, what)

    each("n_streams", n_streams=0)
    each("n_streams", n_streams=257)
    each("workspace", w=None)
    each("workspace", w=ws + 4)
    each("workspace", nbytes=need - 257)                               # a short workspace
    each("workspace", n_streams=S + 1)                                 # sized for fewer streams
    err(lib.cp_online_seq_set_model(S, ws, need, 0, ids, thr, 0, cost, 0, None), sm, "classes")
    err(lib.cp_online_seq_set_model(S, ws, need, 0, ids, thr, 65, cost, 0, None), sm, "classes")
    err(lib.cp_online_seq_set_model(S, ws, need, 0, None, thr, 2, cost, 0, None), sm, "classes")
    err(lib.cp_online_seq_set_model(S, ws, need, 0, ids, None, 2, cost, 0, None), sm, "classes")
    err(lib.cp_online_seq_set_model(S, ws, need, 0, ids, thr, 2, None, 0, None), sm, "cost")
    err(lib.cp_online_seq_set_model(S, ws, need, S, ids, thr, 2, cost, 0, None), sm, "stream index")
    err(lib.cp_online_seq_set_model(S, ws, need, -1, ids, thr, 2, cost, 0, None), sm, "stream index")
    err(lib.cp_online_seq_set_model(S, ws, need, 0, ids, thr, 2, cost, -1, None), sm, "lag")
    err(lib.cp_online_seq_set_model(S, ws, need, 0, ids, thr, 2, cost, 64, None), sm, "lag")
    for bad in ([3, 2], [2, 2], [-1, 4]):                              # unsorted, repeated, negative (-1 is 'none')
        err(lib.cp_online_seq_set_model(S, ws, need, 0, (ctypes.c_int32 * 2)(*bad), thr, 2, cost, 0, None), sm, "ascending")
    nan = (ctypes.c_float * 2)(0.0, float("nan"))
    err(lib.cp_online_seq_set_model(S, ws, need, 0, ids, nan, 2, cost, 0, None), sm, "min_cosine")
    err(lib.cp_online_seq_reset(S, ws, need, S, None), rs, "stream index")
    err(lib.cp_online_seq_reset(S, ws, need, -2, None), rs, "stream index")
    err(lib.cp_online_seq_push(S, ws, need, lg, 2, rows, rows, 65537, out, out, out, None), pu, "total_rows")
    err(lib.cp_online_seq_push(S, ws, need, lg, 2, rows, rows, -1, out, out, out, None), pu, "total_rows")
    err(lib.cp_online_seq_push(S, ws, need, lg, 0, rows, rows, 1, out, out, out, None), pu, "ldl")
    err(lib.cp_online_seq_push(S, ws, need, None, 2, rows, rows, 1, out, out, out, None), pu, "logits")
    err(lib.cp_online_seq_push(S, ws, need, lg, 2, None, rows, 1, out, out, out, None), pu, "row0")
    err(lib.cp_online_seq_push(S, ws, need, lg, 2, rows, None, 1, out, out, out, None), pu, "row0")
    err(lib.cp_online_seq_push(S, ws, need, lg, 2, rows, rows, 1, None, out, out, None), pu, "command")
    assert lib.cp_online_seq_push(S, ws, need, None, 2, None, None, 0, None, None, None, None) == 0        # nothing to do

    cfg = (_lib.cp_online_seq_config * 2)()
    scores = (ctypes.c_int64 * 20)()
    scratch = ctypes.create_string_buffer(256 * 4)
    sb = lib.cp_online_seq_sweep_scratch_bytes(4)

    def sweep(logits=lg, ldl=2, n_rows=4, k=2, exp=rows, costs=cost, n_models=1, configs=cfg, mc=thr, n_configs=2, scr=scratch,
              scr_bytes=sb, sc=scores, cmds=None):
        return lib.cp_online_seq_sweep(logits, ldl, n_rows, k, exp, costs, n_models, configs, mc, n_configs, scr, scr_bytes, sc, cmds,
                                       None)

    err(sweep(k=0), sw, "n_classes")
    err(sweep(k=65, ldl=65), sw, "n_classes")
    err(sweep(ldl=1), sw, "ldl")
    err(sweep(n_configs=0), sw, "n_configs")
    err(sweep(n_configs=65537), sw, "n_configs")
    err(sweep(n_models=0), sw, "n_models")
    err(sweep(n_rows=0), sw, "n_rows")
    err(sweep(n_rows=2 ** 31), sw, "n_rows")
    for name in ("logits", "exp", "costs", "configs", "mc", "scr", "sc"):
        err(sweep(**{name: None}), sw, "required")
    err(sweep(scr_bytes=sb - 1), sw, "scratch too small")
    err(sweep(cmds=ctypes.addressof(scratch) + 2), sw, "misaligned")
