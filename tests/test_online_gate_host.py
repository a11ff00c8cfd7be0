"""CPU checks of the grasp command gate (contrastiveprosthetics_amd/online.py CommandGate, csrc/online_gate.cuh): the numpy
restatement of its semantics that the GPU tests compare against (`GateReference`), `thresholds_from_logits` against a brute-force
loop, the refusals of the cp_online_gate_* entries before any device call, and the wrapper's refusals and resynchronisation
through a stub decoder."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
GATE = ["cp_online_gate_workspace_bytes", "cp_online_gate_set_classes", "cp_online_gate_reset", "cp_online_gate_push"]
ERR_ARG = 10001
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# the semantics of include/cpnative.h, restated: one stream, one window at a time, f32 arithmetic, integer weights
# ---------------------------------------------------------------------------------------------------------------------------
class GateReference:
    """One stream of the gate.  `events` counts what the state machine did, so that a test can show its input made it work."""
    EVENTS = ("rejected_cosine", "rejected_margin", "blocked_min_votes", "switch_after_dwell", "pending_broken", "release")

    def __init__(self, ids, min_cosine, vote, min_votes=1, dwell=1, release=1, weight="count", min_margin=0.0):
        self.vote, self.min_votes, self.dwell, self.release = int(vote), int(min_votes), int(dwell), int(release)
        self.weight, self.min_margin = weight, F(min_margin)
        self.command = -1                        # class id, or -1
        self.events = dict.fromkeys(self.EVENTS, 0)
        self.set_classes(ids, min_cosine)

    def set_classes(self, ids, min_cosine):
        self.ids = [int(i) for i in ids]
        assert self.ids == sorted(set(self.ids)) and self.ids[0] >= 0
        thr = np.broadcast_to(np.asarray(min_cosine, dtype=F), (len(self.ids),))
        self.thr = thr.copy()
        self.ring = []                           # (slot or -1, weight), oldest first
        self.pending, self.run = -1, 0           # run == 0: nothing is pending
        if self.command not in self.ids:
            self.command = -1

    def reset(self):
        self.ring, self.pending, self.run, self.command = [], -1, 0, -1

    def state(self):
        return dict(ring=list(self.ring), pending=self.pending if self.run else None, run=self.run, command=self.command)

    def step(self, row):
        """row (K,) f32 -> (command, accepted, conf, margin)"""
        row = np.asarray(row, dtype=F)
        K = len(self.ids)
        assert row.shape == (K,)
        ev = self.events
        k1 = int(np.argmax(row)) if np.isfinite(row).all() else 0          # first maximum
        if not np.isfinite(row).all():
            slot, w, accepted, conf, margin = -1, 1, -1, F(np.nan), F(np.nan)
        else:
            c1 = row[k1]
            c2 = F(-1.0) if K == 1 else np.max(np.delete(row, k1))
            margin = F(c1 - c2)
            conf = c1
            w = 1 if self.weight == "count" else 1 + int(np.rint(F(min(margin, F(2.0)) * F(2.0 ** 20))))
            ok_cos, ok_margin = bool(c1 >= self.thr[k1]), bool(margin >= self.min_margin)
            ev["rejected_cosine"] += not ok_cos
            ev["rejected_margin"] += ok_cos and not ok_margin
            slot = k1 if ok_cos and ok_margin else -1
            accepted = self.ids[k1] if slot >= 0 else -1
        self.ring.append((slot, w))
        if len(self.ring) > self.vote:
            self.ring.pop(0)
        count, weight = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        for s, x in self.ring:
            if s >= 0:
                count[s] += 1
                weight[s] += x
        cand = -1
        for k in range(K):                       # the largest weight among the qualified; ties: the smallest slot
            if count[k] >= self.min_votes and (cand < 0 or weight[k] > weight[cand]):
                cand = k
        if cand < 0 and count.max() > 0:
            ev["blocked_min_votes"] += 1
        cand_id = self.ids[cand] if cand >= 0 else -1
        if cand_id == self.command or (cand < 0 and self.release == 0):
            ev["pending_broken"] += self.run > 0
            self.run = 0
        elif self.run > 0 and cand == self.pending:
            self.run += 1
        else:
            ev["pending_broken"] += self.run > 0
            self.pending, self.run = cand, 1
        if self.run > 0 and self.run >= (self.dwell if self.pending >= 0 else self.release):
            if self.pending >= 0:
                ev["switch_after_dwell"] += 1
            else:
                ev["release"] += 1
            self.command = self.ids[self.pending] if self.pending >= 0 else -1
            self.run = 0
        return self.command, accepted, conf, margin

    def run_rows(self, logits):
        """(M, K) -> command, accepted (M,) int32 and conf, margin (M,) f32"""
        out = [self.step(r) for r in np.asarray(logits, dtype=F)]
        if not out:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, F), np.zeros(0, F)
        c, a, f, m = zip(*out)
        return np.array(c, np.int32), np.array(a, np.int32), np.array(f, F), np.array(m, F)


def test_reference_with_every_gate_open_is_the_mode_of_the_ring():
    """the third consequence of the semantics, on the restatement itself: all gates open -> command = the vote of the decoders
    (mode of the last `vote` first maxima, ties to the smallest id)"""
    rng = np.random.default_rng(0)
    for K, vote in ((1, 3), (2, 25), (41, 25), (64, 256), (5, 1)):
        ids = np.sort(rng.choice(200, K, replace=False))
        ref = GateReference(ids, -2.0, vote)
        lg = rng.uniform(-1, 1, (600, K)).astype(F)
        lg[rng.random(600) < 0.2] = F(0.25)                   # whole rows of ties
        cmd, acc, conf, margin = ref.run_rows(lg)
        pred = lg.argmax(1)
        for j in range(600):
            win = pred[max(0, j + 1 - vote):j + 1]
            cnt = np.bincount(win, minlength=K)
            assert cmd[j] == ids[int(np.argmax(cnt))], (K, vote, j)
            assert acc[j] == ids[pred[j]] and conf[j] == lg[j].max()
        assert not any(ref.events[k] for k in ("rejected_cosine", "rejected_margin", "blocked_min_votes", "release"))


def test_reference_dwell_release_and_hold():
    ids, K = [3, 7, 9], 3

    def rows(seq):                                 # a clear winner per window; -1: a window nothing wins
        out = np.full((len(seq), K), -0.5, dtype=F)
        for j, s in enumerate(seq):
            if s >= 0:
                out[j, s] = 0.9
        return out

    ref = GateReference(ids, 0.5, vote=1, dwell=3, release=2)
    cmd = ref.run_rows(rows([0, 0, 0, 1, 1, 0, 1, 1, 1, -1, 1, -1, -1, 2]))[0]
    assert cmd.tolist() == [-1, -1, 3, 3, 3, 3, 3, 3, 7, 7, 7, 7, -1, -1]
    assert ref.events["switch_after_dwell"] == 2 and ref.events["release"] == 1 and ref.events["pending_broken"] >= 2
    ref = GateReference(ids, 0.5, vote=1, dwell=1, release=0)              # never release: none leaves the command alone
    assert ref.run_rows(rows([-1, 2, -1, -1, -1, 0]))[0].tolist() == [-1, 9, 9, 9, 9, 3]
    ref.set_classes([3, 4], 0.5)                   # the command's id survives; the ring is empty
    assert ref.state() == dict(ring=[], pending=None, run=0, command=3)
    ref.set_classes([4, 9], 0.5)
    assert ref.command == -1


def test_reference_margin_weights_are_integers_and_outvote_counts():
    ref = GateReference([0, 1], -2.0, vote=3, weight="margin")
    lg = np.array([[0.9, -0.9], [0.1, 0.2], [0.1, 0.2]], dtype=F)         # one sure window against two unsure ones
    assert ref.run_rows(lg)[0].tolist() == [0, 0, 0]
    assert ref.ring[0][1] == 1 + int(np.rint(F(F(0.9) - F(-0.9)) * F(2 ** 20)))
    ref = GateReference([0, 1], -2.0, vote=3, weight="count")
    assert ref.run_rows(lg)[0].tolist() == [0, 0, 1]
    big = GateReference([0, 1], -2.0, vote=256, weight="margin")
    big.run_rows(np.tile(np.array([[1.0, -1.0]], dtype=F), (256, 1)))
    assert sum(w for _, w in big.ring) == 256 * (2 ** 21 + 1) < 2 ** 31


# ---------------------------------------------------------------------------------------------------------------------------
# thresholds_from_logits
# ---------------------------------------------------------------------------------------------------------------------------
def test_thresholds_from_logits_against_a_brute_force_loop():
    from contrastiveprosthetics_amd.online import thresholds_from_logits
    rng = np.random.default_rng(1)
    for keep in (0.95, 0.5, 1.0, 0.9):
        ids = np.array([2, 5, 11, 40])
        lg = rng.uniform(-1, 1, (500, 4)).astype(F)
        lab = rng.choice([-1, 2, 5, 11, 7], 500)                # 40 never cued, 7 not a column
        got = thresholds_from_logits(lg, lab, ids, keep=keep)
        want = {}
        for k, c in enumerate(ids):
            v = []
            for j in range(500):
                if lab[j] == c and all(lg[j, k] > lg[j, q] for q in range(k)) and all(lg[j, k] >= lg[j, q] for q in range(k, 4)):
                    v.append(float(lg[j, k]))
            if v:
                v.sort()
                want[int(c)] = v[int(np.floor((1.0 - keep) * len(v)))]
        assert got == want and 40 not in got and len(got) == 3, (keep, got, want)
    assert thresholds_from_logits(np.zeros((0, 2), F), np.zeros(0, int), [0, 1]) == {}
    with pytest.raises(ValueError):
        thresholds_from_logits(lg, lab, ids, keep=0.0)
    with pytest.raises(ValueError):
        thresholds_from_logits(lg, lab[:-1], ids)
    with pytest.raises(ValueError):
        thresholds_from_logits(lg, lab, ids[:-1])


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def test_gate_symbols_declared_exported_and_bound(lib):
    from contrastiveprosthetics_amd import _lib
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in GATE:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    body = hdr[hdr.index("typedef struct cp_online_gate_config {"):hdr.index("} cp_online_gate_config;")]
    fields = re.findall(r"\b(?:int32_t|float)\s+(\w+);", body)
    assert fields == [f[0] for f in _lib.cp_online_gate_config._fields_] == ["vote", "min_votes", "dwell", "release", "weight",
                                                                            "min_margin"]
    assert ctypes.sizeof(_lib.cp_online_gate_config) == 24


def test_gate_workspace_is_per_stream_state(lib):
    one = lib.cp_online_gate_workspace_bytes(1)
    # K, ids[64], min_cosine[64], ring slots [256] and weights [256], head, len, command, pending, run
    assert one >= 4 * (1 + 64 + 64 + 256 + 256 + 5) and one % 256 == 0
    sizes = [lib.cp_online_gate_workspace_bytes(s) for s in (1, 2, 64, 256)]
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3] <= 256 * one
    assert lib.cp_online_gate_workspace_bytes(0) == one


def _gcfg(**kw):
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_gate_config()
    cfg.vote, cfg.min_votes, cfg.dwell, cfg.release, cfg.weight, cfg.min_margin = 25, 1, 1, 1, 0, 0.0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_gate_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory as the 'workspace': every refusal returns before a launch, which on this machine would fail differently"""
    S = 4
    need = lib.cp_online_gate_workspace_bytes(S)
    buf = ctypes.create_string_buffer(need + 256)
    ws = (ctypes.addressof(buf) + 255) // 256 * 256
    ids = (ctypes.c_int32 * 65)(*range(65))
    thr = (ctypes.c_float * 65)()
    rows = (ctypes.c_int32 * S)()
    out = (ctypes.c_int32 * 8)()
    lg = (ctypes.c_float * 64)()

    def calls(cfg, n_streams=S, w=ws, nbytes=need):
        cr = ctypes.byref(cfg)
        return (("cp_online_gate_set_classes", lambda: lib.cp_online_gate_set_classes(cr, n_streams, w, nbytes, 0, ids, thr, 2, None)),
                ("cp_online_gate_reset", lambda: lib.cp_online_gate_reset(cr, n_streams, w, nbytes, -1, None)),
                ("cp_online_gate_push", lambda: lib.cp_online_gate_push(cr, n_streams, w, nbytes, lg, 2, rows, rows, 1, out, out,
                                                                        None, None, None)))

    def err(rc, entry, what):
        assert rc == ERR_ARG, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    def each(cfg, what, **kw):                      # every entry refuses, one at a time (cp_last_error is the last call's)
        for entry, call in calls(cfg, **kw):
            err(call(), entry, what)

    each(_gcfg(vote=0), "vote")
    each(_gcfg(vote=257), "vote")
    each(_gcfg(dwell=0), "dwell")
    each(_gcfg(release=-1), "release")
    each(_gcfg(min_votes=0), "min_votes")
    each(_gcfg(weight=2), "weight")
    each(_gcfg(min_margin=-0.5), "min_margin")
    each(_gcfg(min_margin=float("nan")), "min_margin")
    each(_gcfg(), "n_streams", n_streams=0)
    each(_gcfg(), "n_streams", n_streams=257)
    each(_gcfg(), "workspace", w=None)
    each(_gcfg(), "workspace", w=ws + 4)
    each(_gcfg(), "workspace", nbytes=need - 257)                          # a short workspace
    each(_gcfg(), "workspace", n_streams=S + 1)                            # sized for fewer streams
    cfg = _gcfg()
    cr = ctypes.byref(cfg)
    sc, rs, pu = "cp_online_gate_set_classes", "cp_online_gate_reset", "cp_online_gate_push"
    err(lib.cp_online_gate_set_classes(cr, S, ws, need, 0, ids, thr, 0, None), sc, "classes")
    err(lib.cp_online_gate_set_classes(cr, S, ws, need, 0, ids, thr, 65, None), sc, "classes")
    err(lib.cp_online_gate_set_classes(cr, S, ws, need, 0, None, thr, 2, None), sc, "classes")
    err(lib.cp_online_gate_set_classes(cr, S, ws, need, S, ids, thr, 2, None), sc, "stream index")
    err(lib.cp_online_gate_set_classes(cr, S, ws, need, -1, ids, thr, 2, None), sc, "stream index")
    for bad in ([3, 2], [2, 2], [-1, 4]):                                 # unsorted, repeated, negative (-1 is 'none')
        err(lib.cp_online_gate_set_classes(cr, S, ws, need, 0, (ctypes.c_int32 * 2)(*bad), thr, 2, None), sc, "ascending")
    nan = (ctypes.c_float * 2)(0.0, float("nan"))
    err(lib.cp_online_gate_set_classes(cr, S, ws, need, 0, ids, nan, 2, None), sc, "min_cosine")
    err(lib.cp_online_gate_reset(cr, S, ws, need, S, None), rs, "stream index")
    err(lib.cp_online_gate_reset(cr, S, ws, need, -2, None), rs, "stream index")
    err(lib.cp_online_gate_push(cr, S, ws, need, lg, 2, rows, rows, 65537, out, out, None, None, None), pu, "total_rows")
    err(lib.cp_online_gate_push(cr, S, ws, need, lg, 2, rows, rows, -1, out, out, None, None, None), pu, "total_rows")
    err(lib.cp_online_gate_push(cr, S, ws, need, lg, 0, rows, rows, 1, out, out, None, None, None), pu, "ldl")
    err(lib.cp_online_gate_push(cr, S, ws, need, None, 2, rows, rows, 1, out, out, None, None, None), pu, "logits")
    err(lib.cp_online_gate_push(cr, S, ws, need, lg, 2, None, rows, 1, out, out, None, None, None), pu, "row0")
    err(lib.cp_online_gate_push(cr, S, ws, need, lg, 2, rows, rows, 1, None, out, None, None, None), pu, "command")
    assert lib.cp_online_gate_push(cr, S, ws, need, None, 2, None, None, 0, None, None, None, None, None) == 0     # nothing to do


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper, through a stub decoder: what it refuses, and when it installs classes again
# ---------------------------------------------------------------------------------------------------------------------------
class StubDecoder:
    """what CommandGate reads of a single-stream decoder"""

    def __init__(self, ids=(1, 4, 6), vote=25):
        import torch
        self.class_ids = torch.tensor(ids, dtype=torch.int32)
        self.n_seen, self.vote, self.phase = 0, vote, 0
        self.pushes = 0

    def push(self, raw, return_logits=False, return_windows=False):
        import torch
        assert return_logits
        self.pushes += 1
        m = raw.shape[0] // 20
        self.n_seen += raw.shape[0]
        k = self.class_ids.numel()
        out = (torch.zeros(m, dtype=torch.int32), torch.ones(m, dtype=torch.int32), torch.zeros(m, k))
        return out + ((torch.zeros(m, 12),) if return_windows else ())

    def reset(self):
        self.n_seen = 0


class StubMulti:
    def __init__(self, n=3):
        self.class_ids = [None] * n
        self._seen = np.zeros(n, dtype=np.int64)
        self.vote, self.phase = 7, 0

    @property
    def n_seen(self):
        return self._seen.copy()

    def push(self, chunks, return_logits=False, return_windows=False):
        import torch
        out = []
        for s, c in enumerate(chunks):
            n = 0 if c is None else c.shape[0]
            self._seen[s] += n
            k = 0 if self.class_ids[s] is None else self.class_ids[s].numel()
            out.append((torch.zeros(n // 20, dtype=torch.int32),) * 2 + (torch.zeros(n // 20, k),))
        return out


def _recording_gate(decoder, **kw):
    """a CommandGate whose three device methods record their calls instead of launching"""
    import torch
    from contrastiveprosthetics_amd.online import CommandGate

    class Recording(CommandGate):
        def __init__(self, *a, **k):
            self.log = []
            super().__init__(*a, **k)

        def _dev_set_classes(self, s, ids, thr):
            self.log.append(("set_classes", s, ids.tolist(), thr.tolist()))

        def _dev_reset(self, s):
            self.log.append(("reset", s))

        def _dev_push(self, ptr, ldl, row0, m, rows):
            self.log.append(("push", ldl, row0.tolist(), m.tolist(), rows))
            return torch.zeros(2, rows, dtype=torch.int32), torch.zeros(2, rows, dtype=torch.float32)

    return Recording(decoder, **kw)


def test_wrapper_refuses_bad_settings():
    from contrastiveprosthetics_amd.online import CommandGate
    dec = StubDecoder()
    for kw in (dict(vote=0), dict(vote=257), dict(dwell=0), dict(release=-1), dict(min_votes=0), dict(weight="sum"),
               dict(min_margin=-1.0), dict(min_margin=float("nan")), dict(min_cosine=float("nan")), dict(min_cosine={1: float("nan")}),
               dict(dwell=1.5)):
        with pytest.raises(ValueError):
            CommandGate(dec, **kw)
    with pytest.raises(TypeError):
        CommandGate(object())
    g = CommandGate(dec, dwell=4, weight="margin")
    assert g.vote == 25 and not g.multi and g.n_streams == 1         # vote defaults to the decoder's
    with pytest.raises(ValueError, match="vote"):
        g.set(vote=3)
    with pytest.raises(TypeError):
        g.set(min_cosine=0.1)
    with pytest.raises(ValueError):
        g.set(release=-2)
    assert (g._cfg.dwell, g._cfg.weight, g._cfg.release) == (4, 1, 1)    # a refused set() changes nothing
    g.set(dwell=2, release=0, min_margin=0.25, weight="count", min_votes=3)
    assert (g._cfg.dwell, g._cfg.release, g._cfg.min_margin, g._cfg.weight, g._cfg.min_votes) == (2, 0, 0.25, 0, 3)
    with pytest.raises(TypeError):
        g.set_thresholds(0, 0.5)                                       # a stream index on a single-stream decoder
    with pytest.raises(TypeError):
        g.push_packed(None, [1])


def test_wrapper_installs_classes_when_the_decoder_replaces_them():
    import torch
    dec = StubDecoder()
    g = _recording_gate(dec, min_cosine={4: 0.5, 99: 0.9}, default=0.125)
    raw = torch.zeros(60, 12)
    out = g.push(raw)
    assert len(out) == 6 and all(o.shape[0] == 3 for o in out)          # pred, voted, command, accepted, conf, margin
    assert g.log == [("set_classes", 0, [1, 4, 6], [0.125, 0.5, 0.125]), ("push", 3, [0], [3], 3)]
    g.push(raw)
    assert [x[0] for x in g.log] == ["set_classes", "push", "push"]      # the same class_ids object: nothing to install
    dec.class_ids = torch.tensor([4, 99], dtype=torch.int32)             # what set_classes / enroll / refresh do
    out = g.push(raw, return_logits=True, return_windows=True)
    assert len(out) == 8 and out[2].shape == (3, 2) and out[3].shape == (3, 12)
    assert g.log[3:] == [("set_classes", 0, [4, 99], [0.5, float(np.float32(0.9))]), ("push", 2, [0], [3], 3)]
    g.set_thresholds(0.75)                                               # new thresholds go in with the next launch
    g.push(raw)
    assert g.log[5] == ("set_classes", 0, [4, 99], [0.75, 0.75]) and g.log[6][0] == "push"
    dec.class_ids = torch.tensor([6, 2], dtype=torch.int32)              # not ascending: refused before the decoder is pushed
    n = dec.pushes
    with pytest.raises(ValueError):
        g.push(raw)
    assert dec.pushes == n


def test_wrapper_raises_when_the_decoder_moved_behind_it():
    import torch
    from contrastiveprosthetics_amd._lib import CpNativeError
    dec = StubDecoder()
    g = _recording_gate(dec)
    raw = torch.zeros(40, 12)
    g.push(raw)
    dec.push(raw, return_logits=True)                                    # behind the gate's back
    n, log = dec.pushes, list(g.log)
    with pytest.raises(CpNativeError, match="behind"):
        g.push(raw)
    assert dec.pushes == n and g.log == log                              # before anything is enqueued
    g.reset()                                                            # the way back: both start a new stream
    assert dec.n_seen == 0 and g.log[-1] == ("reset", -1)
    g.push(raw)
    dec.reset()
    with pytest.raises(CpNativeError, match="behind"):
        g.push(raw)
    # apply() takes the caller's own logits, so the caller pushes the decoder: it re-reads n_seen and does not raise
    lg = dec.push(raw, return_logits=True)[2]
    cmd, acc, conf, margin = g.apply(lg)
    assert cmd.shape == (2,) and g.log[-1] == ("push", 3, [0], [2], 2)
    g.push(raw)
    with pytest.raises(ValueError, match="columns"):
        g.apply(torch.zeros(2, 5))


def test_wrapper_splits_long_pushes_and_packs_streams():
    import torch
    dec = StubDecoder()
    g = _recording_gate(dec)
    out = g.push(torch.zeros(20 * 600, 12))                              # 600 windows: launches of at most 256 rows
    assert [x[3] for x in g.log if x[0] == "push"] == [[256], [256], [88]] and out[2].shape == (600,)
    m = StubMulti(3)
    gm = _recording_gate(m)
    assert gm.multi and gm.n_streams == 3 and gm.vote == 7
    m.class_ids[0] = torch.tensor([0, 1], dtype=torch.int32)
    m.class_ids[2] = torch.tensor([5, 6, 7], dtype=torch.int32)
    gm.set_thresholds(2, {6: 0.5})
    res = gm.push([torch.zeros(40, 12), None, torch.zeros(20, 12)])
    assert [x[:2] for x in gm.log[:2]] == [("set_classes", 0), ("set_classes", 2)] and gm.log[1][3] == [-2.0, 0.5, -2.0]
    assert gm.log[2] == ("push", 64, [0, 2, 2], [2, 0, 1], 3)            # separate tensors: packed into (rows, 64)
    assert [len(r) for r in res] == [6, 6, 6] and [r[2].shape[0] for r in res] == [2, 0, 1]
    with pytest.raises(Exception, match="no class list"):
        gm.apply([None, torch.zeros(1, 2), None])
    with pytest.raises(IndexError):
        gm.set_thresholds(3, 0.5)
    with pytest.raises(ValueError):
        gm.apply([None, None])
    # the packed logits of a multi-stream push are taken as they lie: one buffer, leading dimension 64
    packed = torch.zeros(3, 64)
    views = [packed[0:2, :2], None, packed[2:3, :3]]
    gm.apply(views)
    assert gm.log[-1] == ("push", 64, [0, 2, 2], [2, 0, 1], 3)
    base, ldl = gm._packed([packed[0:2, :2], None, packed[2:3, :3]], np.array([0, 2, 2]))
    assert base.data_ptr() == packed.data_ptr() and ldl == 64


def test_gate_exported_lazily():
    import contrastiveprosthetics_amd as pkg
    from contrastiveprosthetics_amd.online import CommandGate, thresholds_from_logits
    assert pkg.CommandGate is CommandGate and pkg.thresholds_from_logits is thresholds_from_logits
