"""Posture prototypes: several class rows per grasp on the GPU.

Everything from `calibrate` to `search_grasp_sets` takes one grasp to be one direction in the 16-d space: `enroll` gives a class
the unit vector of the sum of its windows.  The same grasp made with the arm down, reaching forward or overhead lands in
different places (the limb-position effect), and the mean of those places can sit on top of another grasp's row.  This module
keeps a row per arm position and answers with the grasp: `fit_prototypes` finds up to four rows per class from a cued
recording's embeddings (cp_online_proto_fit, csrc/online_prototypes.cuh), `Prototypes.install` writes them into a decoder as
rows with ids of their own, and `PostureRows` is a stage behind that decoder, as `CommandGate` is, that turns its row logits
back into class logits, a class prediction and a class vote (cp_online_group_*).  `fit_reference` and `group_reference` are
the definitions, in numpy with every operation rounded on its own (no fused multiply-add); the device equals them in every
integer and bit.  Every dot product is the f32 sum over d = 0..15, in that order, from 0.

The fit.  embeddings e (M, 16) f32 (z / |z| as a push emits it, `track.embed_recording`); expected (M,) per window (class id,
REST, IGNORE); ids (K,) ascending; rows_per_class R_c in 1..4, their sum at most 64; iters in 0..64; min_windows >= 1; use
(M,) bool, optional: the windows that may train.  The windows of class slot c are those with expected == ids[c], `use` set and
all 16 components finite, in window order.  Per class:

centre 0.  S = the float64 sum of the windows in window order, |S| the float64 root of the squares summed with d ascending;
centre 0 = float32(S / |S|), the row `enroll` writes for a zero prior at mix = 1.  A class with fewer than min_windows windows
or |S| = 0 is not fitted: no rows, counts 0, assign -1.
centres 1..R_c-1, farthest-first.  near(i) starts at -inf and takes every dot product of window i with the centres chosen so
far that is > it; the next centre is the window with the smallest near (-0 equals +0), the earliest among equals, copied bit
for bit.
`iters` Lloyd rounds.  Each window goes to the centre with the largest dot product, the first maximum under `>` from centre 0;
per centre the float64 sum in window order and the count; a centre with count > 0 and |S| > 0 becomes float32(S / |S|),
otherwise it stays.  moved[c][t] counts the windows whose centre differs from the round before, in round 0 every window.  A
round that moves nothing leaves a fixed point: the rows stop changing.
final assignment against the final centres: counts[c][q], and assign[i], the row index within the class, -1 for a window that
did not train.  valid[c][q] = counts[c][q] >= min_windows; a centre that is not valid is dropped, a class with no valid centre
counts as not fitted.

Rows in a decoder.  Row q of class id c gets the row id 4 * c + q (`row_id`; `class_of_row` is the inverse), so row ids are
distinct and sorting by id keeps a class's rows adjacent.  The table holds the valid fitted rows, and for a class that was not
fitted the decoder's current row under the id 4 * c.

The stage, per window, in window order: the class logit of a group is the first maximum under `>` of its rows' logits in row
order (the f32 maximum), NaN if one of them is a NaN; a window with a row logit that is not finite predicts nothing (pred and
row -1; its class logits are written by the same rule, +-inf included); otherwise pred is the group with the largest class
logit, the smallest among equals, and row the id of that group's first maximum.  pred enters the decoders' vote ring (a "none"
takes a place and does not vote); voted is the group with the most entries, the smallest among equals, -1 if none has one.

Nothing here is about real subjects; `posture_recording` is a synthetic person.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from .holdout import _logits, _unit_rows, _vote_ring
from .track import _expected_slots, _host, _ids_array

REST, IGNORE = -1, -2                   # online.REST, online.IGNORE
D_E = _lib.CP_D_E
MAX_CLASSES = _lib.CP_ONLINE_MAX_CLASSES
MAX_VOTE = _lib.CP_ONLINE_MAX_VOTE
MAX_ROWS = _lib.CP_ONLINE_PROTO_MAX_ROWS
MAX_ITERS = _lib.CP_ONLINE_PROTO_MAX_ITERS
VOTE = 25                               # online.VOTE
_OPG_WORDS = 4 + 3 * MAX_CLASSES + MAX_VOTE          # OpgState in 32-bit words (csrc/online_prototypes.cuh; asserted in online_api.cuh)


def row_id(class_id: int, q: int) -> int:
    """The id of row q (0..3) of class `class_id` in a decoder's table."""
    if not 0 <= int(q) < MAX_ROWS:
        raise ValueError(f"a class has rows 0..{MAX_ROWS - 1}")
    return MAX_ROWS * int(class_id) + int(q)


def class_of_row(row: int) -> int:
    """The class id of a row id: the inverse of `row_id`."""
    return int(row) // MAX_ROWS


# ---------------------------------------------------------------------------------------------------------------------------
# the definitions (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------
def _int(v, what: str, low: int, high: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not low <= int(v) <= high:
        raise ValueError(f"{what} must be an integer in {low}..{high}")
    return int(v)


def _check_fit(ids, rows_per_class, iters, min_windows):
    cid = _ids_array(ids)
    k = int(cid.shape[0])
    if isinstance(rows_per_class, (int, np.integer)) and not isinstance(rows_per_class, bool):
        rpc = np.full(k, int(rows_per_class), dtype=np.int64)
    else:
        rpc = np.asarray(_host(rows_per_class))
        if rpc.dtype.kind not in "iu" or rpc.shape != (k,):
            raise ValueError(f"rows_per_class must be an integer or one integer per id ({k})")
        rpc = rpc.astype(np.int64)
    if (rpc < 1).any() or (rpc > MAX_ROWS).any():
        raise ValueError(f"rows_per_class must lie in 1..{MAX_ROWS}")
    if int(rpc.sum()) > MAX_CLASSES:
        raise ValueError(f"rows_per_class sums to {int(rpc.sum())} rows, a table holds at most {MAX_CLASSES}")
    return cid, rpc.astype(np.int32), _int(iters, "iters", 0, MAX_ITERS), _int(min_windows, "min_windows", 1, 2 ** 31 - 1)


def _use_array(use, m: int) -> Optional[np.ndarray]:
    if use is None:
        return None
    u = _host(use)
    if u.shape != (m,) or u.dtype.kind not in "biu":
        raise ValueError(f"use must hold one boolean entry per window ({m})")
    return u != 0


def _seq_sum(w: np.ndarray) -> np.ndarray:
    """the float64 sum of the rows of w (n, 16) f32 in row order, from 0 (a cumulative sum is sequential)"""
    return np.cumsum(np.concatenate([np.zeros((1, D_E)), w.astype(np.float64)]), axis=0)[-1]


def _norm64(s: np.ndarray) -> np.float64:
    s2 = np.float64(0.0)
    for d in range(D_E):
        s2 = s2 + s[d] * s[d]
    return np.sqrt(s2)


def _first_max(dots: np.ndarray) -> np.ndarray:
    """(n, R) f32 -> (n,) the first maximum under `>` from column 0 (a NaN is never greater, and nothing is greater than one)"""
    best = np.zeros(dots.shape[0], dtype=np.int64)
    bv = dots[:, 0].copy()
    for r in range(1, dots.shape[1]):
        better = dots[:, r] > bv
        bv = np.where(better, dots[:, r], bv)
        best = np.where(better, r, best)
    return best


def fit_reference(embeddings, expected, ids, rows_per_class=2, iters: int = 10, min_windows: int = 25, use=None) -> dict:
    """The definition of the fit (module docstring).  embeddings (M, 16) f32; expected (M,) class ids, REST or IGNORE; ids the
    K ascending class ids; rows_per_class an int or (K,) ints in 1..4, summing to at most 64; iters in 0..64; min_windows >= 1;
    use (M,) bool or None.  Returns a dict: rows (K, 4, 16) f32, counts (K, 4) int64, valid (K, 4) bool, moved (K, iters)
    int64, assign (M,) int32, and ids, rows_per_class, min_windows as they were given.  Host only (numpy)."""
    cid, rpc, iters, minw = _check_fit(ids, rows_per_class, iters, min_windows)
    k = int(cid.shape[0])
    emb = np.array(_host(embeddings), dtype=np.float32)
    if emb.ndim != 2 or emb.shape[1] != D_E:
        raise ValueError("embeddings must be (M, 16) float32")
    m = int(emb.shape[0])
    slots = _expected_slots(expected, m, cid).astype(np.int64)
    usev = _use_array(use, m)
    rows = np.zeros((k, MAX_ROWS, D_E), dtype=np.float32)
    counts = np.zeros((k, MAX_ROWS), dtype=np.int64)
    valid = np.zeros((k, MAX_ROWS), dtype=bool)
    moved = np.zeros((k, iters), dtype=np.int64)
    assign = np.full(m, -1, dtype=np.int32)
    trains = np.isfinite(emb).all(axis=1) if usev is None else np.isfinite(emb).all(axis=1) & usev
    with np.errstate(all="ignore"):
        for c in range(k):
            idx = np.nonzero(trains & (slots == c))[0]
            n = int(idx.shape[0])
            if n < minw:
                continue
            w = emb[idx]
            s = _seq_sum(w)
            sn = _norm64(s)
            if not sn > 0:
                continue
            r_c = int(rpc[c])
            cen = np.zeros((r_c, D_E), dtype=np.float32)
            cen[0] = (s / sn).astype(np.float32)
            for t in range(1, r_c):
                dots = _logits(w, cen[:t])
                near = np.full(n, -np.inf, dtype=np.float32)
                for r in range(t):
                    near = np.where(dots[:, r] > near, dots[:, r], near)
                cen[t] = w[int(np.argmin(near))]               # the first minimum: the earliest window among equals
            prev = None
            for t in range(iters):
                a = _first_max(_logits(w, cen))
                moved[c, t] = n if prev is None else int((a != prev).sum())
                prev = a
                for q in range(r_c):
                    sel = a == q
                    if sel.any():
                        sq = _seq_sum(w[sel])
                        nq = _norm64(sq)
                        if nq > 0:
                            cen[q] = (sq / nq).astype(np.float32)
            a = _first_max(_logits(w, cen))
            assign[idx] = a
            counts[c, :r_c] = np.bincount(a, minlength=r_c)
            rows[c, :r_c] = cen
            valid[c, :r_c] = counts[c, :r_c] >= minw
    return dict(rows=rows, counts=counts, valid=valid, moved=moved, assign=assign, ids=cid, rows_per_class=rpc, min_windows=minw)


def prototype_table(ids, rows, valid, current=None):
    """The table `Prototypes.install` hands to `set_classes`: (table (R, 16) f32, row_ids (R,) int64, ascending).  For class
    slot c the rows[c][q] with valid[c][q] under the ids 4 * ids[c] + q; for a class with no valid row current[c] under the id
    4 * ids[c] (current: (K, 16) f32, the decoder's row of every class, or a dict {class id: row}; a class that needs one and
    has none is a ValueError).  A dropped centre is never in the table.  Host only (numpy)."""
    cid = _ids_array(ids)
    k = int(cid.shape[0])
    if int(cid[-1]) >= (2 ** 31 - 1) // MAX_ROWS:
        raise ValueError(f"class ids must stay below {(2 ** 31 - 1) // MAX_ROWS}: a row id is {MAX_ROWS} * class id + row")
    rw = np.array(_host(rows), dtype=np.float32)
    ok = np.asarray(_host(valid)).astype(bool)
    if rw.shape != (k, MAX_ROWS, D_E) or ok.shape != (k, MAX_ROWS):
        raise ValueError(f"rows (K, {MAX_ROWS}, 16) and valid (K, {MAX_ROWS}) for the K ids")
    table, rid = [], []
    for c in range(k):
        qs = np.nonzero(ok[c])[0]
        if qs.size:
            for q in qs.tolist():
                table.append(rw[c, q])
                rid.append(row_id(cid[c], q))
            continue
        if isinstance(current, dict):
            row = current.get(int(cid[c]))
        else:
            row = None if current is None else np.asarray(_host(current), dtype=np.float32).reshape(-1, D_E)[c]
        if row is None:
            raise ValueError(f"class {int(cid[c])} was not fitted and there is no current row for it")
        table.append(np.asarray(row, dtype=np.float32).reshape(D_E))
        rid.append(row_id(cid[c], 0))
    return np.stack(table).astype(np.float32), np.array(rid, dtype=np.int64)


def row_logits_reference(embeddings, table) -> np.ndarray:
    """(M, R) f32: the logits a decoder's tail gives with `table` (R, 16) installed: the rows normalised as `set_classes`
    does, products and sums rounded one by one.  Host only (numpy)."""
    emb = np.array(_host(embeddings), dtype=np.float32).reshape(-1, D_E)
    with np.errstate(all="ignore"):
        return _logits(emb, _unit_rows(np.array(_host(table), dtype=np.float32).reshape(-1, D_E)))


def _groups(row_ids, mapping):
    """row ids (R,) ascending and a mapping (callable, dict, array of R class ids or None: every row its own class) ->
    (row_ids (R,) int64, class_of_row (R,) int64, group_ids (G,) int64 ascending, group_of (R,) int64)"""
    rid = _ids_array(row_ids)
    if mapping is None:
        cls = rid.copy()
    elif callable(mapping):
        cls = np.array([mapping(int(r)) for r in rid], dtype=object)
    elif isinstance(mapping, dict):
        cls = np.array([mapping.get(int(r), int(r)) for r in rid], dtype=object)
    else:
        cls = np.asarray(_host(mapping)).reshape(-1)
        if cls.shape[0] != rid.shape[0]:
            raise ValueError("class_of_row must hold one class id per row")
    for v in cls.tolist():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2 ** 31 - 1:
            raise ValueError("class_of_row must give class ids in 0..2**31-2")
    cls = cls.astype(np.int64)
    gid, group_of = np.unique(cls, return_inverse=True)
    return rid, cls, gid, group_of.astype(np.int64)


def group_reference(logits, row_ids, class_of_row=class_of_row, vote: int = VOTE) -> dict:
    """The definition of the stage (module docstring) over one stream from an empty ring: logits (M, R) f32, the row logits of
    a decoder whose table rows have the ascending ids row_ids; class_of_row a callable, a dict {row id: class id}, R class ids
    or None (every row its own class).  Returns a dict: pred, voted (M,) int64 class ids, -1 none; row (M,) int64 row id, -1
    none; logits (M, G) f32 class logits; ids (G,) int64 the class ids, ascending.  Host only (numpy)."""
    rid, _, gid, group_of = _groups(row_ids, class_of_row)
    vote = _int(vote, "vote", 1, MAX_VOTE)
    l = np.array(_host(logits), dtype=np.float32)
    if l.ndim != 2 or l.shape[1] != rid.shape[0]:
        raise ValueError(f"logits must be (M, {rid.shape[0]}) float32: one column per row id")
    m, g = int(l.shape[0]), int(gid.shape[0])
    cl = np.zeros((m, g), dtype=np.float32)
    first = np.zeros((m, g), dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(g):
            members = np.nonzero(group_of == j)[0]
            best, br = l[:, members[0]].copy(), np.full(m, members[0], dtype=np.int64)
            for r in members[1:].tolist():
                better = l[:, r] > best
                best = np.where(better, l[:, r], best)
                br = np.where(better, r, br)
            cl[:, j] = np.where(np.isnan(l[:, members]).any(axis=1), np.float32(np.nan), best)
            first[:, j] = br
        good = np.isfinite(l).all(axis=1)
        k1 = np.where(good, np.argmax(np.where(np.isnan(cl), -np.inf, cl), axis=1), -1)
    voted = _vote_ring(k1, g, vote)
    to_id = np.concatenate([gid, [-1]])
    row = np.where(k1 >= 0, rid[first[np.arange(m), np.maximum(k1, 0)]], -1) if m else np.zeros(0, dtype=np.int64)
    return dict(pred=to_id[k1], voted=to_id[voted], row=row.astype(np.int64), logits=cl, ids=gid)


def posture_recording(m: int, k: int, postures: int = 2, seed: int = 0, segment: int = 40, rest: int = 10, noise: float = 0.12,
                      spread: float = 1.0):
    """A synthetic cued recording of a person whose grasp 0 depends on the arm position, for tests and measurements; nothing
    about real subjects.  Returns (embeddings (m, 16) f32 unit rows, expected (m,) int64 class ids 0..k-1 or REST, posture (m,)
    int32, the arm position of each cued window, -1 under REST).  The cue walks through the k classes again and again,
    `segment` windows per cue with `rest` REST windows behind each (noise alone); repetition r is made in arm position
    r % postures.  Class 1 has one centre u in every position; class 0's centre in position p is u + spread * t_p * v with v
    orthogonal to u and t_p spaced evenly over -1..1, so its positions straddle class 1 and their mean falls on u; the other
    classes have one random centre each.  A cued window is its centre plus `noise` * a standard normal vector, normalised.
    Host only; the same arrays for the same arguments."""
    m, k, postures = _int(m, "m", 1, 2 ** 31 - 1), _int(k, "k", 2, MAX_CLASSES), _int(postures, "postures", 1, 32)
    segment, rest = _int(segment, "segment", 1, 2 ** 31 - 1), _int(rest, "rest", 0, 2 ** 31 - 1)
    rng = np.random.default_rng(seed)
    unitv = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    centres = unitv(rng.standard_normal((k, D_E)))
    u = centres[1]
    v = rng.standard_normal(D_E)
    v = unitv(v - (v @ u) * u)
    offsets = np.linspace(-1.0, 1.0, postures) if postures > 1 else np.zeros(1)
    emb = np.zeros((m, D_E))
    exp = np.full(m, REST, dtype=np.int64)
    pos = np.full(m, -1, dtype=np.int32)
    at, rep = 0, 0
    while at < m:
        p = rep % postures
        for c in range(k):
            centre = unitv(u + spread * offsets[p] * v) if c == 0 else centres[c]
            n = min(segment, m - at)
            emb[at:at + n] = unitv(centre + noise * rng.standard_normal((n, D_E)))
            exp[at:at + n], pos[at:at + n] = c, p
            at += n
            n = min(rest, m - at)
            emb[at:at + n] = unitv(rng.standard_normal((n, D_E)))
            at += n
            if at >= m:
                break
        rep += 1
    return emb.astype(np.float32), exp, pos


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
class Prototypes:
    """What a fit found: ids (K,) int64; rows (K, 4, 16) f32; counts (K, 4) int64, valid (K, 4) bool and moved (K, iters) int64
    as numpy; assign (M,) int32; rows_per_class (K,) and min_windows as the fit took them.  rows and assign are on the GPU
    after `fit_prototypes` and numpy after `Prototypes.of(fit_reference(...))`."""

    def __init__(self, ids, rows, counts, valid, moved, assign, rows_per_class, min_windows):
        self.ids = _ids_array(ids)
        self.rows, self.assign = rows, assign
        self.counts = np.asarray(counts, dtype=np.int64)
        self.valid = np.asarray(valid).astype(bool)
        self.moved = np.asarray(moved, dtype=np.int64)
        self.rows_per_class = np.asarray(rows_per_class, dtype=np.int32)
        self.min_windows = int(min_windows)

    @classmethod
    def of(cls, fit: dict) -> "Prototypes":
        """A `Prototypes` from what `fit_reference` returned."""
        return cls(*(fit[key] for key in ("ids", "rows", "counts", "valid", "moved", "assign", "rows_per_class", "min_windows")))

    @property
    def fitted(self) -> np.ndarray:
        """(K,) bool: the classes with at least one valid row."""
        return self.valid.any(axis=1)

    def table(self, current=None):
        """`prototype_table` of this fit: (table (R, 16) f32, row_ids (R,) int64) numpy."""
        return prototype_table(self.ids, self.rows, self.valid, current)

    def install(self, decoder, stream: Optional[int] = None, stage: Optional["PostureRows"] = None) -> "PostureRows":
        """Write the fitted rows into `decoder` (any of the four online decoders; a multi-stream one with `stream`) and return
        the `PostureRows` stage for it.  The table is the valid fitted rows under the row ids 4 * class id + q, plus, for each
        class that was not fitted, the decoder's current row of that class under the row id 4 * class id; it goes in through
        the decoder's own `set_classes(table=..., ids=row_ids)`, which normalises the rows and empties the vote ring.

        Without stage= a new stage is returned.  On a multi-stream decoder it groups only the installed stream by the row-id
        convention; every other stream keeps one class per row (mapping None), which is right for a plain table: give those
        streams their grouping with a later `install(..., stage=)` or `set_class_of_row`.  stage=: an existing stage of this
        decoder, whose grouping of that stream is replaced and which is returned; use it for every install behind the first.

        The current row of a class that was not fitted: without stage= the decoder's ids are taken as class ids, so the
        decoder must hold a plain one-row-per-class table (after an earlier install its ids are row ids: pass that install's
        stage); with stage= the decoder's rows are mapped to classes as the stage maps them and the class's first row is
        taken.  A class that needs a row and has none is a ValueError, before the decoder is touched.

        While such a table is installed, the decoder's own `pred` and `voted` are ROW ids, not class ids, and its logits have
        one column per row; `enroll`, `finetune` and `track.PrototypeTracker` address rows (a label or cue must name a row id,
        and each moves one row on its own).  Class ids, class votes and class logits come from the stage: push and reset
        through it.  `set_classes` with a plain table puts the decoder back to one row per class."""
        import torch
        multi = isinstance(decoder.class_ids, (list, tuple))
        if multi and stream is None:
            raise ValueError("install(decoder, stream) on a multi-stream decoder")
        if stage is not None and stage.decoder is not decoder:
            raise ValueError("stage= must be a PostureRows of this decoder")
        s = 0
        if multi:
            if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < len(decoder.class_ids):
                raise IndexError(f"stream index must be an int in 0..{len(decoder.class_ids) - 1}, got {stream!r}")
            s = int(stream)
        current = None
        if not self.fitted.all():
            current = {}
            ids_now = decoder.class_ids[s] if multi else decoder.class_ids
            if ids_now is not None:
                rows_now = _host((decoder.class_table(s) if multi else decoder.class_table())[0])
                cls_now = _host(ids_now).astype(np.int64)
                if stage is not None:
                    stage._derive()
                    cls_now = stage._groups[s][1]                  # the class of each of the decoder's rows, in row order
                for j in range(cls_now.shape[0] - 1, -1, -1):      # (backwards: the first row of a class stays)
                    current[int(cls_now[j])] = rows_now[j]
        table, rid = self.table(current)
        t = torch.from_numpy(table)
        if multi:
            decoder.set_classes(s, table=t, ids=rid)
        else:
            decoder.set_classes(table=t, ids=rid)
        if stage is None:
            return PostureRows(decoder, [class_of_row if i == s else None for i in range(len(decoder.class_ids))] if multi else class_of_row)
        stage.set_class_of_row(*((s, class_of_row) if multi else (class_of_row,)))
        return stage


def fit_prototypes(embeddings, expected, ids, rows_per_class=2, iters: int = 10, min_windows: int = 25, use=None) -> Prototypes:
    """`fit_reference` on the device, the whole fit in one launch (cp_online_proto_fit: one wave per class).  embeddings
    (M, 16) f32 on the GPU (`track.embed_recording`); the other arguments as `fit_reference` takes them, checked before the
    launch.  Returns a `Prototypes` whose rows (K, 4, 16) f32 and assign (M,) int32 stay on the GPU and whose counts, valid and
    moved are numpy, equal to the definition's.  One host synchronisation: the copy of those three."""
    import ctypes as C
    import torch
    from .holdout import _device_embeddings
    cid, rpc, iters, minw = _check_fit(ids, rows_per_class, iters, min_windows)
    k = int(cid.shape[0])
    emb = _device_embeddings(embeddings)
    m, dev = int(emb.shape[0]), emb.device
    slots = _expected_slots(expected, m, cid)
    usev = _use_array(use, m)
    lib = _lib.load()
    with torch.cuda.device(dev):
        slot_d = torch.from_numpy(slots).to(dev)
        use_d = None if usev is None else torch.from_numpy(usev.astype(np.uint8)).to(dev)
        rows = torch.empty(k, MAX_ROWS, D_E, dtype=torch.float32, device=dev)
        counts_d = torch.empty(k, MAX_ROWS, dtype=torch.int64, device=dev)
        moved_d = torch.empty(k, iters, dtype=torch.int64, device=dev)
        valid_d = torch.empty(k, MAX_ROWS, dtype=torch.uint8, device=dev)
        assign = torch.empty(m, dtype=torch.int32, device=dev)
        _lib.check(lib.cp_online_proto_fit(emb.data_ptr(), m, k, slot_d.data_ptr(), None if use_d is None else use_d.data_ptr(),
                                           (C.c_int32 * k)(*rpc.tolist()), iters, minw, rows.data_ptr(), counts_d.data_ptr(),
                                           valid_d.data_ptr(), moved_d.data_ptr() if iters else None, assign.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream), "cp_online_proto_fit")
        host = torch.cat([counts_d, moved_d, valid_d.to(torch.int64)], dim=1).cpu().numpy()
    return Prototypes(cid, rows, host[:, :MAX_ROWS], host[:, MAX_ROWS + iters:] != 0, host[:, MAX_ROWS:MAX_ROWS + iters], assign, rpc, minw)


class PostureRows:
    """The grasp, not the arm position, from a decoder whose table holds several rows per class: per stream one state machine
    on the device that reads the row logits of every push (include/cpnative.h, cp_online_group_*; one launch more per push for
    any stream count, nothing is copied to the host).  The module docstring has the definition.

    source: any of the four online decoders.  class_of_row: which class a table row belongs to -- a callable row id -> class
    id (default: `class_of_row`, row id // 4, the convention of `Prototypes.install`), a dict {row id: class id} (other rows are
    their own class), or None (every row its own class: pred, voted and the logits are then the decoder's own bit for bit); on
    a multi-stream decoder one of those for every stream, or a list with one per stream.

    The stage exposes what `CommandGate` and `GraspDrive` ask of a decoder -- `class_ids` (the class ids), `n_seen`, `vote`,
    `push`, `push_packed`, `reset`, `device` -- so they stack on it unchanged: `CommandGate(stage)`, `GraspDrive(stage)`.
    `push` returns the decoder's tuple shape, (pred, voted[, logits][, windows]) with class ids and class logits (M, G), and
    with return_rows=True the winning row id per window behind it.  The class logits have the layout that
    `thresholds_from_logits`, `sweep_gate`, `sweep_subsets`, `search_grasp_sets` and `CommandGate.apply` take, with `class_ids`
    as their ids.

    The stage follows the decoder: a new `class_ids` object there (set_classes, install, enroll, finetune, refresh) makes it
    derive its groups again before the next launch -- the ring empties -- and a push or reset of the decoder behind its back
    makes the next `push` raise `CpNativeError` before anything is enqueued."""

    def __init__(self, source, class_of_row=class_of_row):
        for name in ("class_ids", "n_seen", "vote", "push", "ws"):
            if not hasattr(source, name):
                raise TypeError("PostureRows wraps an OnlineDecoder, MultiStreamDecoder or AdaptiveMultiStreamDecoder")
        self.decoder = source
        self.multi = isinstance(source.class_ids, (list, tuple))
        self.n_streams = len(source.class_ids) if self.multi else 1
        self.vote = _int(source.vote, "vote", 1, MAX_VOTE)
        self.device = source.device
        each = list(class_of_row) if isinstance(class_of_row, (list, tuple)) else [class_of_row] * self.n_streams
        if len(each) != self.n_streams:
            raise ValueError(f"class_of_row: one mapping, or a list of {self.n_streams}")
        self._maps = each
        self._rows_seen = [None] * self.n_streams           # the decoder's class_ids object each stream's groups came from
        self._groups = [None] * self.n_streams              # (row_ids, class_of_row, group_ids, group_of)
        self._class_ids = [None] * self.n_streams           # the class ids (G,) int64: a new object with every derivation
        self._dirty = [False] * self.n_streams              # derived on the host, not yet on the device
        self.ws = None                                      # allocated with the first launch
        self._rows_cache = {}
        self._left = self._seen_now()

    # ------------------------------------------------------------------ what a stage stacked on this one asks
    @property
    def n_seen(self):
        return self.decoder.n_seen

    @property
    def class_ids(self):
        """The class ids, ascending: (G,) int64 numpy or None; on a multi-stream decoder a list with one per stream."""
        self._derive()
        return list(self._class_ids) if self.multi else self._class_ids[0]

    def row_ids(self, stream: int = 0) -> Optional[np.ndarray]:
        """The decoder's row ids of one stream, ascending, or None."""
        self._derive()
        g = self._groups[self._index(stream)]
        return None if g is None else g[0].copy()

    def _index(self, stream) -> int:
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {stream!r}")
        return int(stream)

    def set_class_of_row(self, *args):
        """set_class_of_row(mapping) on a single-stream decoder, set_class_of_row(stream, mapping) on a multi-stream one.  It
        goes in with the next launch, as a new class list does: that stream's ring empties."""
        if len(args) != (2 if self.multi else 1):
            raise TypeError("set_class_of_row(stream, mapping) on a multi-stream decoder, set_class_of_row(mapping) otherwise")
        s = self._index(args[0]) if self.multi else 0
        self._maps[s] = args[-1]
        self._rows_seen[s] = None

    # ------------------------------------------------------------------ the device side (one method per C entry)
    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _args(self):
        if self.ws is None:
            import torch
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_group_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return self.vote, self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_set_groups(self, s: int, rid: np.ndarray, cls: np.ndarray):
        import ctypes as C
        r = int(rid.shape[0])
        args = self._args()
        _lib.check(self.lib.cp_online_group_set_groups(*args, s, (C.c_int32 * r)(*rid.tolist()), (C.c_int32 * r)(*cls.tolist()), r,
                                                       self._stream()), "cp_online_group_set_groups")

    def _dev_reset(self, s: int):
        args = self._args()
        _lib.check(self.lib.cp_online_group_reset(*args, s, self._stream()), "cp_online_group_reset")

    def _dev_push(self, logits_ptr: int, ldl: int, row0: np.ndarray, m: np.ndarray, rows: int, want_logits: bool):
        """one launch over `rows` packed rows -> (pred, voted, row) (3, rows) int32 and class logits (rows, 64) f32 or None"""
        import torch
        from .online import _rows_on_device
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.device)
        pvr = torch.empty(3, rows, dtype=torch.int32, device=self.device)
        cl = torch.empty(rows, MAX_CLASSES, dtype=torch.float32, device=self.device) if want_logits else None
        _lib.check(self.lib.cp_online_group_push(*args, logits_ptr, ldl, rm[0].data_ptr(), rm[1].data_ptr(), rows, pvr[0].data_ptr(),
                                                 pvr[1].data_ptr(), pvr[2].data_ptr(), cl.data_ptr() if want_logits else None,
                                                 MAX_CLASSES if want_logits else 0, self._stream()),
                   "cp_online_group_push")
        return pvr, cl

    # ------------------------------------------------------------------ staying in step with the decoder
    def _seen_now(self) -> np.ndarray:
        return np.array(self.decoder.n_seen, dtype=np.int64).reshape(-1).copy()

    def _decoder_ids(self, s: int):
        return self.decoder.class_ids[s] if self.multi else self.decoder.class_ids

    def _derive(self):
        """the groups of every stream whose decoder holds a new `class_ids` object, on the host"""
        for s in range(self.n_streams):
            cur = self._decoder_ids(s)
            if cur is None or cur is self._rows_seen[s]:
                continue
            g = _groups(_host(cur), self._maps[s])
            self._groups[s], self._class_ids[s] = g, g[2]
            self._rows_seen[s] = cur
            self._dirty[s] = True

    def _sync_groups(self):
        self._derive()
        for s in range(self.n_streams):
            if self._dirty[s]:
                self._dev_set_groups(s, self._groups[s][0], self._groups[s][1])
                self._dirty[s] = False

    def _check_in_step(self):
        if not np.array_equal(self._seen_now(), self._left):
            raise _lib.CpNativeError("the decoder was pushed or reset behind the posture stage (its n_seen is not what the stage "
                                     "left): the stage's ring no longer follows the stream; push and reset through the stage, or "
                                     "reset() it")

    # ------------------------------------------------------------------ the stage over per-stream row logits
    def _stage(self, per_stream, trusted: bool = False, want_logits: bool = True):
        """per_stream: n_streams entries, None or (M_s, R_s) f32 row logits -> per stream (pred, voted, row, class logits or
        None)"""
        import torch
        from .online import _packed_rows
        self._sync_groups()
        step = _lib.CP_ONLINE_MAX_WINDOWS
        ms = []
        for s, t in enumerate(per_stream):
            if t is None:
                ms.append(0)
                continue
            if not trusted:
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.device.type != "cuda":
                    raise ValueError("logits must be (M, R) float32 tensors on the GPU")
                if t.shape[0] and self._groups[s] is None:
                    raise _lib.CpNativeError(f"stream {s} has logits but no class list: set_classes on the decoder first")
                if t.shape[0] and t.shape[1] != self._groups[s][0].shape[0]:
                    raise ValueError(f"stream {s}: logits have {t.shape[1]} columns, its table {self._groups[s][0].shape[0]} rows")
            ms.append(int(t.shape[0]))
        width = [0 if g is None else int(g[2].shape[0]) for g in self._groups]
        outs = []                                              # per round: per stream (pred, voted, row, class logits)
        for lo in range(0, max(max(ms), 1), step):
            m = np.array([min(max(n - lo, 0), step) for n in ms], dtype=np.int64)
            rows = int(m.sum())
            row0 = np.zeros_like(m)
            np.cumsum(m[:-1], out=row0[1:])
            if rows == 0:
                pvr = torch.empty(3, 0, dtype=torch.int32, device=self.device)
                cl = torch.empty(0, MAX_CLASSES, dtype=torch.float32, device=self.device) if want_logits else None
            else:
                whole = lo == 0 and max(ms) <= step
                views = [None if n == 0 else (per_stream[s] if whole else per_stream[s][lo:lo + n]) for s, n in enumerate(m.tolist())]
                base, ldl = _packed_rows(views, row0, trusted, MAX_CLASSES)
                pvr, cl = self._dev_push(base.data_ptr(), ldl, row0, m, rows, want_logits)
            ml = m.tolist()
            outs.append(list(zip(pvr[0].split(ml), pvr[1].split(ml), pvr[2].split(ml),
                                 [None] * self.n_streams if cl is None else [x[:, :w] for x, w in zip(cl.split(ml), width)])))
        if len(outs) == 1:
            return outs[0]
        return [tuple(None if outs[0][s][i] is None else torch.cat([o[s][i] for o in outs]) for i in range(4))
                for s in range(self.n_streams)]

    # ------------------------------------------------------------------ API
    def apply(self, logits):
        """The stage alone on row logits the caller already has (of the decoder's next windows, in order): (M, R) f32 on the
        GPU -> (pred, voted, row, class_logits); on a multi-stream decoder a list with one entry per stream (None: no windows)
        -> one such tuple per stream.  pred, voted (M,) int32 class ids or -1, row (M,) int32 row id or -1, class_logits (M, G)
        f32."""
        import torch
        if self.multi:
            if isinstance(logits, torch.Tensor) or len(logits) != self.n_streams:
                raise ValueError(f"logits must be a sequence of {self.n_streams} entries (None or (M, R) tensors)")
            out = self._stage(list(logits))
        else:
            out = self._stage([logits])[0]
        self._left = self._seen_now()
        return out

    @staticmethod
    def _pick(res, t, return_logits: bool, return_windows: bool, return_rows: bool):
        out = [t[0], t[1]]
        if return_logits:
            out.append(t[3])
        if return_windows:
            out.append(res[3])
        if return_rows:
            out.append(t[2])
        return tuple(out)

    def push(self, raw, return_logits: bool = False, return_windows: bool = False, return_rows: bool = False):
        """What the decoder's `push` takes (raw (n, 12), or one chunk per stream) -> (pred, voted[, logits][, windows][, row])
        per stream: class ids, class logits (M, G), and the winning row id of every window."""
        self._check_in_step()
        self._sync_groups()
        res = self.decoder.push(raw, return_logits=True, return_windows=return_windows)
        return self._finish(res, return_logits, return_windows, return_rows)

    def push_packed(self, raw, counts, return_logits: bool = False, return_windows: bool = False, return_rows: bool = False):
        """`push` for samples packed in stream order, as the multi-stream decoders' `push_packed`."""
        if not self.multi:
            raise TypeError("push_packed belongs to the multi-stream decoders")
        self._check_in_step()
        self._sync_groups()
        res = self.decoder.push_packed(raw, counts, return_logits=True, return_windows=return_windows)
        return self._finish(res, return_logits, return_windows, return_rows)

    def _finish(self, res, return_logits: bool, return_windows: bool, return_rows: bool):
        self._left = self._seen_now()
        if self.multi:
            staged = self._stage([r[2] for r in res], trusted=True, want_logits=return_logits)
            return [self._pick(r, t, return_logits, return_windows, return_rows) for r, t in zip(res, staged)]
        return self._pick(res, self._stage([res[2]], trusted=True, want_logits=return_logits)[0], return_logits, return_windows, return_rows)

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back (this waits for the device; a test and debugging aid): row_ids,
        group_of (the group slot of each row), class_ids, and ring, the group slots (-1: none) from the oldest to the newest.
        The layout is that of OpgState (csrc/online_prototypes.cuh): int32 R, G, head, len, row_ids[64], group_of[64],
        group_ids[64], ring[256]."""
        import torch
        s = self._index(stream)
        if self.ws is None:
            return dict(row_ids=[], group_of=[], class_ids=[], ring=[])
        w = self.ws[:self.n_streams * _OPG_WORDS * 4].view(torch.int32).reshape(self.n_streams, _OPG_WORDS)[s].cpu().numpy()
        r, g, head, n = (int(x) for x in w[:4])
        ring = w[4 + 3 * MAX_CLASSES:]
        return dict(row_ids=w[4:4 + r].tolist(), group_of=w[4 + MAX_CLASSES:4 + MAX_CLASSES + r].tolist(),
                    class_ids=w[4 + 2 * MAX_CLASSES:4 + 2 * MAX_CLASSES + g].tolist(),
                    ring=[int(ring[(head - n + i) % self.vote]) for i in range(n)])

    def reset(self, streams=None):
        """Reset the decoder and the stage's ring (the groups stay); on a multi-stream decoder the listed streams, default
        all."""
        self._sync_groups()
        if self.multi and streams is not None:
            idx = sorted({self._index(s) for s in streams})
            self.decoder.reset(idx)
            for s in idx:
                self._dev_reset(s)
        else:
            self.decoder.reset()
            self._dev_reset(-1)
        self._left = self._seen_now()
