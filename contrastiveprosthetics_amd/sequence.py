"""Grasp sequence decoder: fixed-lag Viterbi behind the logits of the online decoders (include/cpnative.h, cp_online_seq_*;
csrc/online_sequence.cuh).

`CommandGate` counts hard votes and turns them into a command through a state machine of six coupled integers.  This stage is
the standard sequence model of sEMG post-processing instead: a transition cost between the grasps and the state "none of
these", evidence summed over time rather than counted, and a decision that may look a few windows ahead.

`SequenceGate` wraps any of the four decoders (or a `PostureRows` / `MetricRows` stage, through `apply` on their class logits)
and keeps one Viterbi state per stream on the device: one launch more per push, nothing is copied to the host.  `potts` and
`transitions_from_cues` build cost matrices; `sweep_sequence` scores many (matrix, thresholds, lag) over a cued recording in one
pass on the device with the ten counters of `score_commands`, so `pick_gate` picks from its table unchanged.
`SequenceReference` is the definition in numpy: everything is int32 arithmetic on quantised cosines, so it and the device agree
in every bit.

To drive a hand, feed the command to the drive: `GraspDrive(decoder, follow='pred').apply(windows, command)` with the windows
and the command of the same push.
"""
from __future__ import annotations

import ctypes as C
import itertools
import numpy as np
import torch

from . import _lib
from .online import (IGNORE, MAX_CLASSES, REST, SCORE_KEYS, CommandGate, _cue_slots, _ids_array, _OnStream, _packed_rows,
                     _rows_on_device)

ONE = 1 << 20                            # a cosine of 1.0 in the stage's integer units
FLOOR = _lib.CP_ONLINE_SEQ_FLOOR         # scores lie in [FLOOR, 0]
MAX_COST = _lib.CP_ONLINE_SEQ_MAX_COST   # "as good as forbidden"
MAX_LAG = _lib.CP_ONLINE_SEQ_RING - 1
_POTTS_KEYS = ("switch", "engage", "release", "through_rest")
_SEQ_KEYS = ("transitions", "min_cosine", "default", "lag")


def quantise(x) -> np.ndarray:
    """q(x) = (int32) rint(min(max(x, -2), 2) * 2^20) in f32: half-even, and the product is exact (NaN -> 0; a row with one is
    flagged before q is used)."""
    v = np.clip(np.nan_to_num(np.asarray(x, dtype=np.float32), nan=0.0), np.float32(-2.0), np.float32(2.0))
    return np.rint(v * np.float32(ONE)).astype(np.int32)


def _cost_units(x, what: str) -> int:
    v = float(x)
    if not (np.isfinite(v) and v >= 0.0):
        raise ValueError(f"{what} must be finite and >= 0 (cosine units)")
    return int(min(np.rint(v * ONE), MAX_COST))


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_CLASSES:
        raise ValueError(f"k must be an int in 1..{MAX_CLASSES}")
    return int(k)


def _check_lag(lag) -> int:
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 0 <= int(lag) <= MAX_LAG:
        raise ValueError(f"lag must be an int in 0..{MAX_LAG}")
    return int(lag)


def potts(k: int, switch: float, engage: float, release: float, through_rest: bool = False) -> np.ndarray:
    """The (k+1, k+1) int32 cost matrix with three prices, in cosine units, quantised with rint(x * 2^20) (at most 2^28): `switch`
    from a grasp to another one, `engage` from none (row and column k) to a grasp, `release` from a grasp to none; staying costs 0.
    through_rest=True: grasp -> another grasp costs 2^28, so a change goes through none (in Ninapro's protocol every movement
    returns to rest)."""
    k = _check_k(k)
    sw, en, rl = _cost_units(switch, "switch"), _cost_units(engage, "engage"), _cost_units(release, "release")
    c = np.full((k + 1, k + 1), MAX_COST if through_rest else sw, dtype=np.int32)
    c[k, :] = en
    c[:, k] = rl
    c[np.arange(k + 1), np.arange(k + 1)] = 0
    return c


def transitions_from_cues(expected, ids, scale: float, floor_count=1) -> np.ndarray:
    """A (K+1, K+1) int32 cost matrix from the transition counts of a cued recording: expected (M,) as `expected_commands` gives
    it (class ids, REST -> the none state, IGNORE breaks a pair), ids the K ascending class ids.  counts[i][j] = the windows in
    state j right behind a window in state i, each with `floor_count` added; p = counts / their row sum; cost = rint(-ln(p) *
    scale * 2^20), clipped to 0..2^28, each row then less its minimum.  A row without any count costs 0.  Host only (numpy)."""
    cid = _ids_array(ids)
    k = cid.shape[0]
    exp = np.asarray(expected.detach().cpu() if isinstance(expected, torch.Tensor) else expected)
    if exp.ndim != 1 or exp.dtype.kind not in "iu":
        raise ValueError("expected must hold one integer entry per window")
    exp = exp.astype(np.int64)
    pos = np.minimum(np.searchsorted(cid, exp), k - 1)
    if ((exp >= 0) & (cid[pos] != exp)).any() or (exp < IGNORE).any():
        raise ValueError("expected holds class ids among ids, REST or IGNORE")
    sc, fc = float(scale), float(floor_count)
    if not (np.isfinite(sc) and sc > 0.0):
        raise ValueError("scale must be finite and > 0")
    if not (np.isfinite(fc) and fc >= 0.0):
        raise ValueError("floor_count must be finite and >= 0")
    state = np.where(exp >= 0, pos, np.where(exp == REST, k, -1))
    pair = (state[:-1] >= 0) & (state[1:] >= 0)
    counts = np.zeros((k + 1, k + 1), dtype=np.float64)
    np.add.at(counts, (state[:-1][pair], state[1:][pair]), 1.0)
    counts += fc
    total = counts.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        cost = -np.log(counts / total) * sc * ONE
    cost = np.where(total > 0, cost, 0.0)
    cost = np.clip(np.rint(np.minimum(cost, float(MAX_COST))), 0, MAX_COST).astype(np.int64)
    return (cost - cost.min(axis=1, keepdims=True)).astype(np.int32)


def _check_matrix(c, k: int) -> np.ndarray:
    c = np.asarray(c.detach().cpu() if isinstance(c, torch.Tensor) else c)
    if c.dtype.kind not in "iu" or c.shape != (k + 1, k + 1):
        raise ValueError(f"a transition matrix for {k} classes is a ({k + 1}, {k + 1}) integer array")
    if (c < 0).any() or (c > MAX_COST).any():
        raise ValueError("transition costs lie in 0..2**28 (units of 2**-20)")
    return np.ascontiguousarray(c, dtype=np.int32)


def _check_transitions(t):
    """a transitions entry as given: the dict `potts` takes, a callable ids -> matrix, or a matrix; ValueError otherwise"""
    if isinstance(t, dict):
        extra = set(t) - set(_POTTS_KEYS)
        if extra:
            raise ValueError(f"a transitions dict takes {', '.join(_POTTS_KEYS)}, not {sorted(extra, key=str)[0]!r}")
        missing = [k for k in _POTTS_KEYS[:3] if k not in t]
        if missing:
            raise ValueError(f"a transitions dict names switch, engage and release; {missing[0]!r} is missing")
        potts(1, **t)                                          # the values, checked now
        return dict(t)
    if callable(t):
        return t
    c = np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t)
    if c.dtype.kind not in "iu" or c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 2:
        raise ValueError("transitions is the dict potts takes, a callable ids -> (K+1, K+1) integer array, or such an array")
    return c


def _matrix_for(t, cid: np.ndarray) -> np.ndarray:
    k = int(cid.shape[0])
    if isinstance(t, dict):
        return potts(k, **t)
    return _check_matrix(t(cid.copy()) if callable(t) else t, k)


class SequenceReference:
    """The definition of the stage in numpy (include/cpnative.h states it in words): one stream.  ids (K,) ascending class ids,
    min_cosine a float or (K,) floats, cost a (K+1, K+1) integer matrix with entries in 0..2^28 (row and column K: none), lag in
    0..63.  `run_rows(logits)` takes the next windows of the stream and returns (command, now, lead) as int32 arrays (class ids
    or -1; lead in units of 2^-20).  `score` (K+1,) int32, `n` and `ring`, the last <= 64 back-pointer rows (K+1,) from the
    oldest to the newest (entries are slots, K: none), are the state."""

    def __init__(self, ids, min_cosine, cost, lag: int = 0):
        self.ids = _ids_array(ids)
        self.K = k = int(self.ids.shape[0])
        thr = np.broadcast_to(np.asarray(min_cosine, dtype=np.float32), (k,))
        if np.isnan(thr).any():
            raise ValueError("min_cosine must not be NaN")
        self.thr = quantise(thr).astype(np.int64)
        self.C = _check_matrix(cost, k).astype(np.int64)
        self.lag = _check_lag(lag)
        self.reset()

    def reset(self):
        self.score = np.zeros(self.K + 1, dtype=np.int32)
        self.ring = []
        self._rows = []                                        # the ring's rows as lists, for the traceback
        self.n = 0

    def _emissions(self, lg: np.ndarray) -> np.ndarray:
        """(M, K) f32 logits -> e (M, K+1) int64: q(l) - thr, 0 in a row with a non-finite logit and for none"""
        e = np.zeros((lg.shape[0], self.K + 1), dtype=np.int64)
        e[:, :self.K] = np.where(np.isfinite(lg).all(axis=1)[:, None], quantise(lg).astype(np.int64) - self.thr, 0)
        return e

    def _advance(self, e: np.ndarray):
        """one window with emissions e (K+1,) -> (command slot, now slot, lead), slot K for none"""
        v = self.score.astype(np.int64)[:, None] - self.C      # v[i][j]
        bp = v.argmax(axis=0)                                  # the smallest i among equals: class slots before none
        new = v.max(axis=0) + e
        new = np.maximum(new - new.max(), FLOOR)
        now = int(new.argmax())
        lead = int(new[now] - np.partition(new, -2)[-2])       # (the runner-up: the second largest entry, equal ones included)
        self.score = new.astype(np.int32)
        self.ring.append(bp.astype(np.int32))
        self._rows.append(bp.tolist())
        del self.ring[:-_lib.CP_ONLINE_SEQ_RING], self._rows[:-_lib.CP_ONLINE_SEQ_RING]
        self.n = min(self.n + 1, 1 << 30)
        if self.n <= self.lag:
            return self.K, now, lead
        s = now
        for t in range(1, self.lag + 1):
            s = self._rows[-t][s]
        return s, now, lead

    def step(self, row):
        """one window: row (K,) f32 logits -> (command slot, now slot, lead), slot K for none"""
        return self._advance(self._emissions(np.asarray(row, dtype=np.float32).reshape(1, self.K))[0])

    def run_rows(self, logits):
        lg = np.asarray(logits.detach().cpu() if isinstance(logits, torch.Tensor) else logits, dtype=np.float32).reshape(-1, self.K)
        out = np.array([self._advance(e) for e in self._emissions(lg)], dtype=np.int64).reshape(-1, 3)
        table = np.concatenate([self.ids, [-1]])
        return table[out[:, 0]].astype(np.int32), table[out[:, 1]].astype(np.int32), out[:, 2].astype(np.int32)


class SequenceGate(_OnStream):
    """A command a hand can follow, from any of the four decoders, by fixed-lag Viterbi decoding: per stream one state on the
    device that reads the logits of every push (include/cpnative.h, cp_online_seq_*; one launch more per push, nothing is
    copied to the host).

    The states are the decoder's classes and "none".  Per window a class gains its cosine less `min_cosine` of that class (none
    gains 0), moving from state i to state j costs `transitions[i][j]`, and the score of the best path into each state is kept.
    `now` is the state with the best score, `lead` its distance to the runner-up, and `command` the state the best path was in
    `lag` windows ago (lag 0: command = now; the first `lag` windows of a stream command none).

    transitions: the dict `potts` takes (switch, engage, release[, through_rest], in cosine units) or a callable
    ids -> (K+1, K+1) integer matrix (units of 2^-20, row and column K the none state), so that a new class list can be
    followed; default potts(0.5, 0.5, 0.5).  min_cosine: one float, or {class id: float} with `default` for the other ids.
    lag: one int in 0..63, or on a multi-stream decoder one per stream.

    The stage follows the decoder as `CommandGate` does: a new `class_ids` object (set_classes, enroll, refresh) is installed
    before the next launch -- the stream restarts -- and a push or reset of the decoder behind the stage's back makes the next
    `push` raise `CpNativeError` before anything is enqueued.  Pushes of more than 256 windows per stream are cut into launches
    of 256.  To drive a hand: `GraspDrive(decoder, follow='pred').apply(windows, command)`."""

    def __init__(self, decoder, transitions=None, min_cosine=-2.0, default: float = -2.0, lag: int = 0):
        for name in ("class_ids", "n_seen", "push"):
            if not hasattr(decoder, name):
                raise TypeError("SequenceGate wraps an OnlineDecoder, MultiStreamDecoder, AdaptiveMultiStreamDecoder or a stage with "
                                "class_ids, n_seen and push")
        self.decoder = decoder
        self.multi = isinstance(decoder.class_ids, (list, tuple))
        self.n_streams = len(decoder.class_ids) if self.multi else 1
        self.transitions = _check_transitions(dict(switch=0.5, engage=0.5, release=0.5) if transitions is None else transitions)
        self._lag = self._check_lags(lag)
        self._thr = [CommandGate._check_thresholds(min_cosine, default)] * self.n_streams
        self._ids_seen = [None] * self.n_streams            # the class_ids object each stream's model was installed from
        self._k = [0] * self.n_streams
        self.device = getattr(decoder, "device", None)
        self.ws = None                                      # allocated with the first launch
        self._rows_cache = {}
        self._left = self._seen_now()

    # ------------------------------------------------------------------ settings
    def _check_lags(self, lag) -> list:
        if isinstance(lag, (list, tuple, np.ndarray)):
            if len(lag) != self.n_streams:
                raise ValueError(f"lag is one int or one per stream ({self.n_streams})")
            return [_check_lag(v) for v in lag]
        return [_check_lag(lag)] * self.n_streams

    @property
    def lag(self):
        """the lag; on a multi-stream decoder the list of the streams' lags"""
        return list(self._lag) if self.multi else self._lag[0]

    def use(self, config: dict):
        """Apply one config of `sweep_sequence` / `sequence_grid` (a dict with the keys transitions, min_cosine, default, lag) to
        every stream; each stream restarts with its next launch.  Nothing changes if a value is refused."""
        extra = set(config) - set(_SEQ_KEYS)
        if extra:
            raise ValueError(f"a sequence config takes {', '.join(_SEQ_KEYS)}, not {sorted(extra, key=str)[0]!r}")
        if "default" in config and "min_cosine" not in config:
            raise ValueError("default goes with min_cosine")
        spec = CommandGate._check_thresholds(config["min_cosine"], config.get("default", -2.0)) if "min_cosine" in config else None
        trans = _check_transitions(config["transitions"]) if "transitions" in config else self.transitions
        lag = self._check_lags(config["lag"]) if "lag" in config else self._lag
        self.transitions, self._lag = trans, lag
        for s in range(self.n_streams):
            if spec is not None:
                self._thr[s] = spec
            self._ids_seen[s] = None

    def set_thresholds(self, *args, default: float = -2.0):
        """set_thresholds(min_cosine) on a single-stream decoder, set_thresholds(stream, min_cosine) on a multi-stream one:
        a float or {class id: float} with `default` for the other ids.  They go in with the next launch, as a new class list
        does: that stream restarts."""
        if len(args) != (2 if self.multi else 1):
            raise TypeError("set_thresholds(stream, min_cosine) on a multi-stream decoder, set_thresholds(min_cosine) otherwise")
        s = self._index(args[0]) if self.multi else 0
        self._thr[s] = CommandGate._check_thresholds(args[-1], default)
        self._ids_seen[s] = None

    def _index(self, stream) -> int:
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {stream!r}")
        return int(stream)

    # ------------------------------------------------------------------ the device side (one method per C entry)
    def _args(self):
        if self.ws is None:
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_seq_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_set_model(self, s: int, ids: np.ndarray, thr: np.ndarray, cost: np.ndarray):
        k = int(ids.shape[0])
        args = self._args()
        cost_d = torch.from_numpy(cost).to(self.ws.device)
        _lib.check(self.lib.cp_online_seq_set_model(*args, s, (C.c_int32 * k)(*ids.tolist()), (C.c_float * k)(*thr.tolist()), k,
                                                    cost_d.data_ptr(), self._lag[s], self._stream()), "cp_online_seq_set_model")

    def _dev_reset(self, s: int):
        args = self._args()
        _lib.check(self.lib.cp_online_seq_reset(*args, s, self._stream()), "cp_online_seq_reset")

    def _dev_push(self, logits_ptr: int, ldl: int, row0: np.ndarray, m: np.ndarray, rows: int) -> torch.Tensor:
        """one launch over `rows` packed rows -> (command, now, lead) as one (3, rows) int32 tensor"""
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.ws.device)
        out = torch.empty(3, rows, dtype=torch.int32, device=self.ws.device)
        _lib.check(self.lib.cp_online_seq_push(*args, logits_ptr, ldl, rm[0].data_ptr(), rm[1].data_ptr(), rows, out[0].data_ptr(),
                                               out[1].data_ptr(), out[2].data_ptr(), self._stream()), "cp_online_seq_push")
        return out

    # ------------------------------------------------------------------ staying in step with the decoder
    def _seen_now(self) -> np.ndarray:
        return np.array(self.decoder.n_seen, dtype=np.int64).reshape(-1).copy()

    def _class_ids(self, s: int):
        return self.decoder.class_ids[s] if self.multi else self.decoder.class_ids

    def _sync_classes(self):
        for s in range(self.n_streams):
            cur = self._class_ids(s)
            if cur is None or cur is self._ids_seen[s]:
                continue
            ids = np.asarray(cur.cpu() if isinstance(cur, torch.Tensor) else cur, dtype=np.int64).reshape(-1)
            if not 1 <= ids.shape[0] <= MAX_CLASSES or (np.diff(ids) <= 0).any() or ids[0] < 0 or ids[-1] >= 2 ** 31 - 1:
                raise ValueError("the stage takes 1..64 ascending class ids in 0..2**31-2 (-1 is its 'none')")
            spec, d = self._thr[s]
            thr = np.array([spec.get(int(i), d) for i in ids], dtype=np.float32)
            self._dev_set_model(s, ids, thr, _matrix_for(self.transitions, ids))
            self._ids_seen[s] = cur
            self._k[s] = int(ids.shape[0])

    def _check_in_step(self):
        if not np.array_equal(self._seen_now(), self._left):
            raise _lib.CpNativeError("the decoder was pushed or reset behind the sequence stage (its n_seen is not what the stage "
                                     "left): its scores no longer follow the stream; push and reset through the stage, or reset() it")

    # ------------------------------------------------------------------ the stage over per-stream logits
    def _decode(self, per_stream, trusted: bool = False):
        """per_stream: n_streams entries, None or (M_s, K_s) f32 logits -> per stream (command, now, lead).
        trusted: the entries are what the decoder's own push just returned (their layout is known, see online._packed_rows)."""
        self._sync_classes()
        step = _lib.CP_ONLINE_MAX_WINDOWS
        ms = []
        for s, t in enumerate(per_stream):
            if t is None:
                ms.append(0)
                continue
            if not trusted:
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
                    raise ValueError("logits must be (M, K) float32 tensors")
                if t.shape[0] and self._ids_seen[s] is None:
                    raise _lib.CpNativeError(f"stream {s} has logits but no class list: set_classes on the decoder first")
                if t.shape[0] and t.shape[1] != self._k[s]:
                    raise ValueError(f"stream {s}: logits have {t.shape[1]} columns, its class list {self._k[s]} ids")
            ms.append(int(t.shape[0]))
        outs = []                                              # per round: per stream (command, now, lead)
        for lo in range(0, max(max(ms), 1), step):
            m = np.array([min(max(n - lo, 0), step) for n in ms], dtype=np.int64)
            rows = int(m.sum())
            row0 = np.zeros_like(m)
            np.cumsum(m[:-1], out=row0[1:])
            if rows == 0:
                dev = next((t.device for t in per_stream if t is not None), self.device)
                out = torch.empty(3, 0, dtype=torch.int32, device=dev)
            else:
                whole = lo == 0 and max(ms) <= step
                views = [None if n == 0 else (per_stream[s] if whole else per_stream[s][lo:lo + n]) for s, n in enumerate(m.tolist())]
                base, ldl = _packed_rows(views, row0, trusted, MAX_CLASSES)
                out = self._dev_push(base.data_ptr(), ldl, row0, m, rows)
            if self.n_streams == 1:
                outs.append([(out[0], out[1], out[2])])
                continue
            ml = m.tolist()
            outs.append(list(zip(out[0].split(ml), out[1].split(ml), out[2].split(ml))))
        if len(outs) == 1:
            return outs[0]
        return [tuple(torch.cat([o[s][i] for o in outs]) for i in range(3)) for s in range(self.n_streams)]

    # ------------------------------------------------------------------ API
    def apply(self, logits):
        """The stage alone on logits the caller already has (of the stream's next windows, in order): (M, K) f32 on the GPU ->
        (command, now, lead); on a multi-stream decoder a list with one entry per stream (None: no windows) -> one such tuple
        per stream.  command, now (M,) int32 class ids or -1; lead (M,) int32 in units of 2^-20."""
        if self.multi:
            if isinstance(logits, torch.Tensor) or len(logits) != self.n_streams:
                raise ValueError(f"logits must be a sequence of {self.n_streams} entries (None or (M, K) tensors)")
            out = self._decode(list(logits))
        else:
            out = self._decode([logits])[0]
        self._left = self._seen_now()
        return out

    @staticmethod
    def _extend(res, decoded, return_logits: bool):
        return tuple(x for i, x in enumerate(res) if i != 2 or return_logits) + tuple(decoded)

    def push(self, raw, return_logits: bool = False, return_windows: bool = False):
        """What the decoder's `push` takes (raw (n, 12), or one chunk per stream) -> the decoder's tuple(s) extended by command,
        now, lead: (pred, voted[, logits][, windows], command, now, lead)."""
        self._check_in_step()
        self._sync_classes()
        res = self.decoder.push(raw, return_logits=True, return_windows=return_windows)
        return self._finish(res, return_logits)

    def push_packed(self, raw, counts, return_logits: bool = False, return_windows: bool = False):
        """`push` for samples packed in stream order, as the multi-stream decoders' `push_packed`."""
        if not self.multi:
            raise TypeError("push_packed belongs to the multi-stream decoders")
        self._check_in_step()
        self._sync_classes()
        res = self.decoder.push_packed(raw, counts, return_logits=True, return_windows=return_windows)
        return self._finish(res, return_logits)

    def _finish(self, res, return_logits: bool):
        self._left = self._seen_now()
        if self.multi:
            decoded = self._decode([r[2] for r in res], trusted=True)
            return [self._extend(r, d, return_logits) for r, d in zip(res, decoded)]
        return self._extend(res, self._decode([res[2]], trusted=True)[0], return_logits)

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back (this waits for the device; a test and debugging aid): score
        (K+1,) int32 (the last entry: none), n, and ring, the last min(n, 64) back-pointer rows (K+1,) int32 from the oldest to
        the newest (entries are slots, K: none) -- what `SequenceReference` keeps under the same names.  The layout is that of
        SqState (csrc/online_sequence.cuh): int32 K, lag, n, head, score of none, C[none][none], 2 unused, ids[64], thr[64],
        C[k][none][64], C[none][k][64], C[64][64], score[64], then 64 ring rows of 68 bytes (column 64: none)."""
        s = self._index(stream)
        if self.ws is None:
            return dict(score=np.zeros(0, dtype=np.int32), n=0, ring=[])
        words, ring_bytes = 8 + 4 * MAX_CLASSES + MAX_CLASSES * MAX_CLASSES + MAX_CLASSES, _lib.CP_ONLINE_SEQ_RING * 68
        per = 4 * words + ring_bytes
        raw = self.ws[s * per:(s + 1) * per].cpu().numpy()
        w = raw[:4 * words].view(np.int32)
        k, n, head = int(w[0]), int(w[2]), int(w[3])
        rows = raw[4 * words:].reshape(_lib.CP_ONLINE_SEQ_RING, 68).astype(np.int32)
        rows = np.where(rows == 64, k, rows)
        keep = min(n, _lib.CP_ONLINE_SEQ_RING)
        at = [(head - keep + i) % _lib.CP_ONLINE_SEQ_RING for i in range(keep)]
        return dict(score=np.concatenate([w[words - MAX_CLASSES:][:k], w[4:5]]).astype(np.int32), n=n,
                    ring=[np.concatenate([rows[i, :k], rows[i, 64:65]]) for i in at])

    def reset(self, streams=None):
        """Reset the decoder and the stage (scores 0, empty ring, n = 0; the models stay); on a multi-stream decoder the listed
        streams, default all."""
        if self.multi and streams is not None:
            idx = sorted({int(s) for s in streams})
            self.decoder.reset(idx)
            for s in idx:
                self._dev_reset(s)
        else:
            self.decoder.reset()
            self._dev_reset(-1)
        self._left = self._seen_now()


# ---------------------------------------------------------------------------------------------------------------------------
# sequence sweep: many (transitions, thresholds, lag) over one cued recording, scored on the device (cp_online_seq_sweep)
# ---------------------------------------------------------------------------------------------------------------------------
def sequence_grid(**lists) -> list:
    """The cartesian product of lists of SequenceGate settings as a list of config dicts, the last name varying fastest:
    sequence_grid(transitions=[a, b], lag=[0, 5]) -> [{transitions: a, lag: 0}, {transitions: a, lag: 5}, {transitions: b, ...}]."""
    extra = set(lists) - set(_SEQ_KEYS)
    if extra:
        raise ValueError(f"a sequence config takes {', '.join(_SEQ_KEYS)}, not {sorted(extra, key=str)[0]!r}")
    names = list(lists)
    return [dict(zip(names, combo)) for combo in itertools.product(*(list(lists[n]) for n in names))]


def _sweep_configs(configs, cid: np.ndarray):
    """configs (dicts with SequenceGate's keys) -> the device arrays' host images: costs (n_models, K+1, K+1) int32 with equal
    matrices stored once, (G, 2) int32 in the layout of cp_online_seq_config, and (G, 64) f32 thresholds per class slot"""
    configs = list(configs)
    if not 1 <= len(configs) <= _lib.CP_ONLINE_SEQ_SWEEP_MAX_CONFIGS:
        raise ValueError(f"sweep_sequence takes 1..{_lib.CP_ONLINE_SEQ_SWEEP_MAX_CONFIGS} configs, got {len(configs)}")
    k = int(cid.shape[0])
    cfg = np.zeros((len(configs), 2), dtype=np.int32)
    thr = np.zeros((len(configs), MAX_CLASSES), dtype=np.float32)
    models, index, by_object = [], {}, {}
    known = set(cid.tolist())
    for g, c in enumerate(configs):
        if not isinstance(c, dict):
            raise ValueError(f"config {g} is not a dict")
        extra = set(c) - set(_SEQ_KEYS)
        if extra:
            raise ValueError(f"config {g}: a sequence config takes {', '.join(_SEQ_KEYS)}, not {sorted(extra, key=str)[0]!r}")
        if "default" in c and "min_cosine" not in c:
            raise ValueError(f"config {g}: default goes with min_cosine")
        t = c.get("transitions", dict(switch=0.5, engage=0.5, release=0.5))
        at = by_object.get(id(t))
        if at is None:
            mat = _matrix_for(_check_transitions(t), cid)
            at = index.setdefault(mat.tobytes(), len(models))
            if at == len(models):
                models.append(mat)
            by_object[id(t)] = at
        spec, d = CommandGate._check_thresholds(c.get("min_cosine", -2.0), c.get("default", -2.0))
        stray = set(spec) - known
        if stray:
            raise ValueError(f"config {g}: min_cosine names class id {sorted(stray)[0]}, which is not among ids")
        cfg[g] = at, _check_lag(c.get("lag", 0))
        thr[g, :k] = [spec.get(int(i), d) for i in cid]
    return np.stack(models), cfg, thr


def _sweep_dev(logits: torch.Tensor, slots: np.ndarray, k: int, costs: np.ndarray, cfg: np.ndarray, thr: np.ndarray, want_commands: bool):
    """the device side of `sweep_sequence` (one call of cp_online_seq_sweep) -> scores (G, 10) int64 on the host, commands (G, M)
    int32 slots on the device or None"""
    lib = _lib.load()
    dev, m, g = logits.device, int(logits.shape[0]), int(cfg.shape[0])
    with torch.cuda.device(dev):
        exp_d, costs_d = torch.from_numpy(slots).to(dev), torch.from_numpy(costs).to(dev)
        cfg_d, thr_d = torch.from_numpy(cfg).to(dev), torch.from_numpy(thr).to(dev)
        scratch = torch.empty(lib.cp_online_seq_sweep_scratch_bytes(m), dtype=torch.uint8, device=dev)
        scores = torch.empty(g, _lib.CP_ONLINE_GATE_SCORES, dtype=torch.int64, device=dev)
        commands = torch.empty(g, m, dtype=torch.int32, device=dev) if want_commands else None
        _lib.check(lib.cp_online_seq_sweep(logits.data_ptr(), int(logits.stride(0)), m, k, exp_d.data_ptr(), costs_d.data_ptr(),
                                           int(costs.shape[0]), cfg_d.data_ptr(), thr_d.data_ptr(), g, scratch.data_ptr(),
                                           scratch.numel(), scores.data_ptr(), commands.data_ptr() if want_commands else None,
                                           torch.cuda.current_stream(dev).cuda_stream), "cp_online_seq_sweep")
        return scores.cpu().numpy(), commands


def sweep_sequence(logits, expected, ids, configs, return_commands: bool = False):
    """Score many SequenceGate settings over one cued recording in one pass on the device (cp_online_seq_sweep: one wave per
    config, each from a fresh state).  logits (M, K) f32 on the GPU, expected (M,) as `expected_commands` gives it, ids the K
    ascending class ids of the columns -- as `sweep_gate` takes them; configs a sequence of dicts with SequenceGate's keys:
    transitions (the dict `potts` takes, a callable ids -> matrix, or a (K+1, K+1) integer matrix; default potts(0.5, 0.5, 0.5)),
    min_cosine (a float or {id: float} with `default`) and lag, checked before anything is enqueued.  Equal matrices are stored
    once.  Returns {key: (G,) int64 array} under SCORE_KEYS, so `pick_gate` picks from it unchanged: config g's entry is
    `score_commands` of the commands a fresh SequenceGate with config g returns for these logits.  return_commands=True:
    (scores, commands) with commands (G, M) int32 on the GPU, class ids or -1.  One host synchronisation: the copy of the table."""
    cid = _ids_array(ids)
    costs, cfg, thr = _sweep_configs(configs, cid)
    slots = _cue_slots(logits, expected, cid)
    g, m = cfg.shape[0], int(logits.shape[0])
    if m == 0:
        scores = np.zeros((g, len(SCORE_KEYS)), dtype=np.int64)
        commands = torch.empty(g, 0, dtype=torch.int32, device=logits.device) if return_commands else None
    else:
        if logits.device.type != "cuda":
            raise ValueError("logits must be on the GPU")
        if logits.stride(1) != 1 or (m > 1 and logits.stride(0) < logits.shape[1]):
            logits = logits.contiguous()
        scores, commands = _sweep_dev(logits, slots, int(cid.shape[0]), costs, cfg, thr, return_commands)
    out = {k: scores[:, i].copy() for i, k in enumerate(SCORE_KEYS)}
    if not return_commands:
        return out
    if m and not np.array_equal(cid, np.arange(cid.shape[0])):        # slots -> class ids, a block of rows at a time
        table = torch.from_numpy(np.concatenate([[-1], cid]).astype(np.int32)).to(commands.device)
        step = max(1, (1 << 24) // m)
        for lo in range(0, g, step):
            commands[lo:lo + step] = table[(commands[lo:lo + step] + 1).long()]
    return out, commands
