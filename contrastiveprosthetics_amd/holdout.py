"""Held-out enrolment scoring: leave-a-repetition-out on the GPU.

Every step behind `enroll` -- `thresholds_from_logits`, `sweep_gate`, `search_grasp_sets`, the tracker sweep -- is scored on the
cued recording whose windows made the class rows, and a cosine prototype scored on its own windows looks better than it is.
This module scores class rows on repetitions they have not seen, for many (training repetitions, held-out repetitions, mix,
min_windows) plans in one pass over the recording's embeddings (cp_online_holdout_*, csrc/online_holdout.cuh).  The encoder is
shared and frozen, so `track.embed_recording` gives z / |z| per window once; from there a held-out table is a masked float64
sum, a blend and a 16-wide dot product per window and class.  `holdout_reference` is the definition, in numpy with every
operation rounded on its own (no fused multiply-add); the device equals it in every integer and bit.

The recording: embeddings e (M, 16) f32; expected (M,) per window, as `online.expected_commands` or `realign.realign_cues`
give it (class id, REST, IGNORE), slot[i] its index into the K ascending ids; rep (M,) the repetition of each window
(`repetitions`), -1 for none.  A plan is a dict: train, eval (bit masks over the repetitions 0..31), mix, min_windows.

Per plan, in this order:

sums.  S[c][d], float64, starts at 0 and takes one add of float64(e[i][d]) per window i in ascending i with slot[i] == c and bit
rep[i] of train set; n[c] counts those windows.  Windows with rep[i] < 0 never train.  This is the accumulator
cp_online_enroll leaves when the same windows are enrolled in order.
row.  The arithmetic of ole_table_kernel (csrc/online_enroll.cuh) with prior[c], mix and min_windows: len = the f32 length of
the prior (sum of squares with d ascending, sqrtf); |S| in float64 likewise; enrolled iff n[c] >= min_windows and |S| > 0;
row = float32((1 - mix) * prior + mix * (len * (S / |S|))), or the prior itself if not enrolled: the row `enroll` installs.
unit row.  As ol_set_classes_kernel: the f32 sum of squares with d ascending, sqrtf, then a divide.
evaluated rows.  The windows in ascending i with bit rep[i] of eval set; rep < 0 is never evaluated.
logits.  l[k] = the f32 sum over d ascending, from 0, of e[i][d] * unit[k][d]: the operations of the decoders' tail.
prediction.  None (-1) if any of the K logits is not finite, else the first maximum under `>`, the lowest slot on ties.
vote.  The decoders' ring, starting empty, runs over the plan's evaluated rows in order and is not cleared at gaps; IGNORE rows
are included; a "none" takes a place and does not vote (the rule of `online.score_subset`).  The voted slot is the most
frequent, the smallest among equals, none if no slot has an entry.
scores.  Nine integers, `HOLDOUT_SCORE_KEYS`: n_cue (evaluated rows with a class cue), pred_hit, voted_hit (the hits among
them), n_rest (evaluated REST rows), n_train (the sum of n[c]), n_enrolled (classes with n[c] >= min_windows), worst_class
(the class with the smallest voted recall among classes with cue rows, fractions compared by cross-multiplication in 64 bits,
the smallest slot among equals; reported as its class id, -1 if there is none), worst_hit, worst_n (its hits and its count).
confusion (K, K): rows = cue slot, columns = predicted slot over the cue rows, "none" not counted; voted_confusion likewise.
sequences: pred and voted per (plan, window) as class ids, -1 for none, `NOT_EVALUATED` (-3) for a window the plan does not
evaluate.

A plan with mix outside [0, 1] or not finite, min_windows < 1 or a mask with bits at or above 32 is refused: it scores -1 in
every counter, its rows stay 0, its confusions 0 and its sequences NOT_EVALUATED.

What was not built: held-out fine-tuning (loop `finetune` with masked labels; the closed-form `readout.pick_ridge` scores a
projection on held-out repetitions), held-out AdaBN calibration, and anything about
real subjects; the person of tools/online_bench.py --holdout is synthetic.
"""
from __future__ import annotations

import itertools
from typing import Optional

import numpy as np

from . import _lib
from .realign import cue_segments
from .track import _expected_slots, _host, _ids_array, embed_recording

REST, IGNORE = -1, -2                   # online.REST, online.IGNORE
NOT_EVALUATED = -3                      # a sequence entry of a window the plan does not evaluate
D_E = _lib.CP_D_E
MAX_CLASSES = _lib.CP_ONLINE_MAX_CLASSES
MAX_VOTE = _lib.CP_ONLINE_MAX_VOTE
MAX_PLANS = _lib.CP_ONLINE_HOLDOUT_MAX_PLANS
MAX_REPS = _lib.CP_ONLINE_HOLDOUT_MAX_REPS
VOTE = 25                               # online.VOTE
ACC_W = 17                              # the accumulator of cp_online_enroll: 16 sums and the count per slot
HOLDOUT_SCORE_KEYS = ("n_cue", "pred_hit", "voted_hit", "n_rest", "n_train", "n_enrolled", "worst_class", "worst_hit", "worst_n")
PLAN_KEYS = ("train", "eval", "mix", "min_windows")
_PLAN_DTYPE = np.dtype([("train", "<u4"), ("eval", "<u4"), ("sums_index", "<i4"), ("min_windows", "<i4"), ("mix", "<f8")])
assert len(HOLDOUT_SCORE_KEYS) == _lib.CP_ONLINE_HOLDOUT_SCORES
# what a decoder's workspace holds in front of its weights (csrc/online_api.cuh, ol_carve; asserted there): per stream an
# OlState, in the multi-stream forms an OlmMeta, in the adaptive forms an OlaHead and the float64 statistics
_OL_STATE_BYTES, _OLM_META_BYTES, _OLA_HEAD_BYTES, _OLA_STATS_BYTES = 7672, 16, 16, 9 * 2 * 512 * 8


# ---------------------------------------------------------------------------------------------------------------------------
# the definition (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------
def repetitions(expected, folds: Optional[int] = None):
    """The repetition of every window of a cued recording: (rep (M,) int32, R).  The cued segments are those of
    `realign.cue_segments`; the r-th segment of a class in time order has repetition r, with folds=F repetition r % F.  A
    window outside every segment takes the repetition of the next segment in time, a window behind the last segment that of
    the last segment.  R is 1 + the largest value; a recording with no segment gives all -1 and R = 0.  More than 32
    repetitions are refused: fold them with folds=.  Host only (numpy)."""
    if folds is not None and (isinstance(folds, bool) or not isinstance(folds, (int, np.integer)) or not 1 <= int(folds) <= MAX_REPS):
        raise ValueError(f"folds must be an integer in 1..{MAX_REPS}")
    exp = _host(expected)
    seg = cue_segments(exp).astype(np.int64)
    m = int(exp.shape[0])
    if seg.shape[0] == 0:
        return np.full(m, -1, dtype=np.int32), 0
    exp = exp.astype(np.int64)
    seen = {}
    seg_rep = np.zeros(seg.shape[0], dtype=np.int64)
    for j, s in enumerate(seg[:, 0].tolist()):
        c = int(exp[s])
        seg_rep[j] = seen.get(c, 0)
        seen[c] = seg_rep[j] + 1
    if folds is not None:
        seg_rep %= int(folds)
    n_rep = int(seg_rep.max()) + 1
    if n_rep > MAX_REPS:
        raise ValueError(f"the recording has {n_rep} repetitions of a class, more than {MAX_REPS}: fold them with folds=")
    nxt = np.searchsorted(seg[:, 1], np.arange(m), side="right")       # the first segment that ends behind the window
    return seg_rep[np.minimum(nxt, seg.shape[0] - 1)].astype(np.int32), n_rep


def _check_reps(n_rep) -> int:
    if isinstance(n_rep, bool) or not isinstance(n_rep, (int, np.integer)) or not 1 <= int(n_rep) <= MAX_REPS:
        raise ValueError(f"the number of repetitions must be an integer in 1..{MAX_REPS}")
    return int(n_rep)


def leave_one_out(n_rep: int, mix: float = 1.0, min_windows: int = 25) -> list:
    """R plans: plan h trains on every repetition but h and evaluates repetition h."""
    r = _check_reps(n_rep)
    full = (1 << r) - 1
    return [dict(train=full & ~(1 << h), eval=1 << h, mix=mix, min_windows=min_windows) for h in range(r)]


def learning_curve(n_rep: int, mix: float = 1.0, min_windows: int = 25) -> list:
    """R (R - 1) plans: for every held-out repetition h and every n in 1..R-1, in this order, train on the n repetitions
    h+1 .. h+n (mod R) and evaluate repetition h."""
    r = _check_reps(n_rep)
    return [dict(train=sum(1 << ((h + j) % r) for j in range(1, n + 1)), eval=1 << h, mix=mix, min_windows=min_windows)
            for h in range(r) for n in range(1, r)]


def plan_grid(plans, mix=None, min_windows=None) -> list:
    """The product of a plan list with lists of `mix` and `min_windows` values (None: the plan's own), the plan varying
    slowest and min_windows fastest."""
    out = []
    for p, mx, mw in itertools.product(list(plans), [None] if mix is None else list(mix), [None] if min_windows is None else list(min_windows)):
        q = dict(p)
        if mx is not None:
            q["mix"] = mx
        if mw is not None:
            q["min_windows"] = mw
        out.append(q)
    return out


def _plan_table(plans):
    """plans -> (train, eval: lists of Python ints, mix (T,) f64, min_windows (T,) int64, ok (T,) bool); ok False: refused"""
    plans = list(plans)
    if not 1 <= len(plans) <= MAX_PLANS:
        raise ValueError(f"1..{MAX_PLANS} plans, got {len(plans)}")
    train, evl = [], []
    mix, minw, ok = np.zeros(len(plans)), np.zeros(len(plans), dtype=np.int64), np.zeros(len(plans), dtype=bool)
    for t, p in enumerate(plans):
        if not isinstance(p, dict) or set(p) - set(PLAN_KEYS) or not {"train", "eval"} <= set(p):
            raise ValueError(f"plan {t} is not a dict with {', '.join(PLAN_KEYS)}")
        for key in ("train", "eval", "min_windows"):
            v = p.get(key, 25)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"plan {t}: {key} must be an integer")
        if abs(int(p.get("min_windows", 25))) >= 2 ** 31:
            raise ValueError(f"plan {t}: min_windows must fit 32 bits")
        train.append(int(p["train"]))
        evl.append(int(p["eval"]))
        mix[t] = float(p.get("mix", 1.0))
        minw[t] = int(p.get("min_windows", 25))
        ok[t] = 0.0 <= mix[t] <= 1.0 and minw[t] >= 1 and 0 <= train[t] < 2 ** MAX_REPS and 0 <= evl[t] < 2 ** MAX_REPS
    return train, evl, mix, minw, ok


def _check_vote(vote) -> int:
    if isinstance(vote, bool) or not isinstance(vote, (int, np.integer)) or not 1 <= int(vote) <= MAX_VOTE:
        raise ValueError(f"vote must lie in 1..{MAX_VOTE}")
    return int(vote)


def _rep_array(rep, m: int) -> np.ndarray:
    r = _host(rep)
    if r.shape != (m,) or r.dtype.kind not in "iu":
        raise ValueError(f"rep must hold one integer entry per window ({m})")
    r = r.astype(np.int64)
    if m and r.max() >= MAX_REPS:
        raise ValueError(f"rep must stay below {MAX_REPS}: fold the repetitions with folds=")
    return np.maximum(r, -1).astype(np.int32)


def _prior_array(prior, k: int) -> np.ndarray:
    p = np.array(_host(prior), dtype=np.float32)
    if p.shape != (k, D_E):
        raise ValueError("prior must hold one row of 16 per id")
    with np.errstate(all="ignore"):
        ss = np.zeros(k, dtype=np.float32)
        for d in range(D_E):
            ss = ss + p[:, d] * p[:, d]
    if not (np.isfinite(ss) & (ss > 0)).all():
        raise ValueError("every prior row must have a finite, non-zero length")
    return p


def _bit(mask: int, rep: np.ndarray) -> np.ndarray:
    """bit rep[i] of mask, False where rep[i] < 0"""
    table = np.array([(mask >> r) & 1 for r in range(MAX_REPS)] + [0], dtype=bool)
    return table[rep]                                      # (-1 reads the last entry)


def _unit_rows(rows: np.ndarray) -> np.ndarray:
    ss = np.zeros(rows.shape[:-1], dtype=np.float32)
    for d in range(D_E):
        ss = ss + rows[..., d] * rows[..., d]
    return rows / np.sqrt(ss)[..., None]


def _logits(emb: np.ndarray, unit: np.ndarray) -> np.ndarray:
    """emb (n, 16), unit (K, 16) or (n, K, 16) f32 -> (n, K) f32: products and sums rounded one by one, d ascending, from 0"""
    u = unit if unit.ndim == 3 else unit[None]
    l = np.zeros((emb.shape[0], u.shape[1]), dtype=np.float32)
    for d in range(D_E):
        l = l + emb[:, d, None] * u[:, :, d]
    return l


def _vote_ring(pred: np.ndarray, k: int, vote: int) -> np.ndarray:
    n = pred.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    entered = np.zeros((n, k), dtype=np.int64)
    entered[np.nonzero(pred >= 0)[0], pred[pred >= 0]] = 1
    in_ring = np.cumsum(entered, axis=0)                   # per slot, entries among the last `vote` evaluated rows
    in_ring[vote:] -= in_ring[:-vote].copy()
    return np.where(in_ring.max(axis=1) > 0, in_ring.argmax(axis=1), -1)


def holdout_reference(embeddings, expected, ids, rep, prior, plans, vote: int = VOTE, return_sequences: bool = False) -> dict:
    """The definition of held-out enrolment scoring (module docstring).  embeddings (M, 16) f32; expected (M,) class ids, REST
    or IGNORE; ids the K ascending class ids; rep (M,) the repetition of each window, below 32, negative: none; prior (K, 16)
    f32 rows of non-zero length; plans a sequence of 1..4096 plan dicts.  Returns a dict: `HOLDOUT_SCORE_KEYS` -> (T,) int64;
    sums (T, K, 16) f64 and counts (T, K) int64; rows, unit (T, K, 16) f32; confusion, voted_confusion (T, K, K) int32; with
    return_sequences pred, voted (T, M) int64 class ids, -1 none, -3 not evaluated.  Host only (numpy)."""
    cid = _ids_array(ids)
    k = int(cid.shape[0])
    vote = _check_vote(vote)
    emb = np.array(_host(embeddings), dtype=np.float32)
    if emb.ndim != 2 or emb.shape[1] != D_E:
        raise ValueError("embeddings must be (M, 16) float32")
    m = int(emb.shape[0])
    slots = _expected_slots(expected, m, cid).astype(np.int64)
    rp = _rep_array(rep, m)
    pr = _prior_array(prior, k)
    train, evl, mix, minw, ok = _plan_table(plans)
    n_plans = len(train)
    out = {key: np.full(n_plans, -1, dtype=np.int64) for key in HOLDOUT_SCORE_KEYS}
    sums, counts = np.zeros((n_plans, k, D_E)), np.zeros((n_plans, k), dtype=np.int64)
    rows, unit = (np.zeros((n_plans, k, D_E), dtype=np.float32) for _ in range(2))
    conf, vconf = (np.zeros((n_plans, k, k), dtype=np.int32) for _ in range(2))
    seq_p, seq_v = (np.full((n_plans, m), NOT_EVALUATED, dtype=np.int64) for _ in range(2))
    e64 = emb.astype(np.float64)
    ss = np.zeros(k, dtype=np.float32)
    for d in range(D_E):
        ss = ss + pr[:, d] * pr[:, d]
    length = np.sqrt(ss).astype(np.float64)
    to_id = np.concatenate([cid, [-1]])
    with np.errstate(all="ignore"):
        for t in range(n_plans):
            if not ok[t]:
                continue
            trains = _bit(train[t], rp) & (slots >= 0)
            for c in range(k):
                sel = trains & (slots == c)
                counts[t, c] = sel.sum()                       # a cumulative sum is sequential; it starts from 0
                sums[t, c] = np.cumsum(np.concatenate([np.zeros((1, D_E)), e64[sel]]), axis=0)[-1]
            s2 = np.zeros(k)
            for d in range(D_E):
                s2 = s2 + sums[t, :, d] * sums[t, :, d]
            sn = np.sqrt(s2)
            enrolled = (counts[t].astype(np.float64) >= np.float64(minw[t])) & (sn > 0)
            blend = (np.float64(1.0) - mix[t]) * pr.astype(np.float64) + mix[t] * (length[:, None] * (sums[t] / sn[:, None]))
            rows[t] = np.where(enrolled[:, None], blend.astype(np.float32), pr)
            unit[t] = _unit_rows(rows[t])
            ev = np.nonzero(_bit(evl[t], rp))[0]
            l = _logits(emb[ev], unit[t])
            pred = np.where(np.isfinite(l).all(axis=1), np.argmax(np.where(np.isnan(l), -np.inf, l), axis=1), -1)
            voted = _vote_ring(pred, k, vote)
            e = slots[ev]
            cue = e >= 0
            n_c = np.bincount(e[cue], minlength=k)
            hit_c = np.bincount(e[cue & (voted == e)], minlength=k)
            worst = -1
            for c in np.nonzero(n_c)[0].tolist():
                if worst < 0 or int(hit_c[c]) * int(n_c[worst]) < int(hit_c[worst]) * int(n_c[c]):
                    worst = c
            sc = (cue.sum(), (cue & (pred == e)).sum(), hit_c.sum(), (e == REST).sum(), counts[t].sum(), (counts[t] >= minw[t]).sum(),
                  cid[worst] if worst >= 0 else -1, hit_c[worst] if worst >= 0 else 0, n_c[worst] if worst >= 0 else 0)
            for key, v in zip(HOLDOUT_SCORE_KEYS, sc):
                out[key][t] = int(v)
            np.add.at(conf[t], (e[cue & (pred >= 0)], pred[cue & (pred >= 0)]), 1)
            np.add.at(vconf[t], (e[cue & (voted >= 0)], voted[cue & (voted >= 0)]), 1)
            seq_p[t, ev], seq_v[t, ev] = to_id[pred], to_id[voted]
    out.update(sums=sums, counts=counts, rows=rows, unit=unit, confusion=conf, voted_confusion=vconf)
    if return_sequences:
        out.update(pred=seq_p, voted=seq_v)
    return out


def cued_recording(k: int, reps: int, segment: int = 60, rest: int = 20, seed: int = 0, noise: float = 0.35, wander: float = 0.3,
                   ids=None):
    """A synthetic cued recording for tests and measurements; nothing about real subjects.  Returns (embeddings (M, 16) f32
    unit rows, expected (M,) int64 class ids or REST, prior (k, 16) f32 unit rows).  The cue walks through the k classes `reps`
    times, `segment` rows per cue with `rest` REST rows behind each (0: none).  A class has a true direction; the prior row is
    that direction disturbed by `wander` * a standard normal vector (the model's row before enrolment), each repetition has a
    direction of its own, disturbed likewise by wander / 2, and a cued row is its repetition's direction plus `noise` * a
    standard normal vector, normalised; a REST row is noise alone.  Host only; the same arrays for the same arguments."""
    rng = np.random.default_rng(seed)
    cid = np.arange(k, dtype=np.int64) if ids is None else _ids_array(ids)
    unitv = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    true = unitv(rng.standard_normal((k, D_E)))
    prior = unitv(true + wander * rng.standard_normal((k, D_E))).astype(np.float32)
    emb, exp = [], []
    for _ in range(reps):
        for c in range(k):
            centre = unitv(true[c] + 0.5 * wander * rng.standard_normal(D_E))
            emb.append(unitv(centre + noise * rng.standard_normal((segment, D_E))))
            exp.append(np.full(segment, cid[c]))
            if rest:
                emb.append(unitv(rng.standard_normal((rest, D_E))))
                exp.append(np.full(rest, REST))
    return np.concatenate(emb).astype(np.float32), np.concatenate(exp).astype(np.int64), prior


def assign_folds(rep, plans, most_trained: bool = False) -> np.ndarray:
    """(M,) int32: for every window the first plan whose `eval` holds the window's repetition, -1 if there is none (also for
    rep < 0 and for refused plans).  most_trained=True: among the plans that hold it, the first with the most training
    repetitions (of a learning curve: the leave-one-out plan of each repetition)."""
    r = _host(rep)
    rp = _rep_array(r, int(r.shape[0]))
    train, evl, _, _, ok = _plan_table(plans)
    order = range(len(train))
    if most_trained:
        order = sorted(order, key=lambda t: (-bin(train[t]).count("1"), t))
    pick = np.full(MAX_REPS + 1, -1, dtype=np.int32)
    for t in order:
        if not ok[t]:
            continue
        for b in range(MAX_REPS):
            if (evl[t] >> b) & 1 and pick[b] < 0:
                pick[b] = t
    return pick[rp]


def holdout_logits_reference(embeddings, unit_rows, assign) -> np.ndarray:
    """(M, K) f32: window i against the unit rows unit_rows[assign[i]] ((T, K, 16) f32, taken as they are), summed as the
    decoders' tail sums them; NaN in the rows with assign[i] outside 0..T-1.  Host only (numpy)."""
    emb = np.array(_host(embeddings), dtype=np.float32).reshape(-1, D_E)
    unit = np.array(_host(unit_rows), dtype=np.float32)
    a = np.asarray(_host(assign)).astype(np.int64).reshape(-1)
    if unit.ndim != 3 or unit.shape[2] != D_E or a.shape[0] != emb.shape[0]:
        raise ValueError("unit_rows (T, K, 16) and one assignment per window")
    has = (a >= 0) & (a < unit.shape[0])
    out = np.full((emb.shape[0], unit.shape[1]), np.nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        out[has] = _logits(emb[has], unit[a[has]])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
def _device_embeddings(embeddings):
    import torch
    if not isinstance(embeddings, torch.Tensor) or embeddings.dtype != torch.float32 or embeddings.dim() != 2 \
            or embeddings.shape[1] != D_E or embeddings.shape[0] < 1:
        raise ValueError("embeddings must be an (M, 16) float32 tensor with at least one row")
    if embeddings.device.type != "cuda":
        raise ValueError("embeddings must be on the GPU")
    emb = embeddings.contiguous()
    return emb.clone() if emb.data_ptr() % 16 else emb


def score_plans(embeddings, expected, ids, rep, prior, plans, vote: int = VOTE, confusion: bool = False,
                return_sequences: bool = False) -> dict:
    """`holdout_reference` on the device, all plans in one pass: cp_online_holdout_sums over the distinct training masks,
    cp_online_holdout_tables, cp_online_holdout_score (one wave per plan).  embeddings (M, 16) f32 on the GPU
    (`track.embed_recording`); the other arguments as `holdout_reference` takes them, checked before the first launch.
    Returns a dict: `HOLDOUT_SCORE_KEYS` -> (T,) int64 numpy, equal to the definition's; on the GPU rows and unit (T, K, 16)
    f32, sums (U, 64, 17) f64 in the accumulator layout of cp_online_enroll with sums_index (T,) numpy naming each plan's;
    confusion=True: confusion, voted_confusion (T, K, K) int32; return_sequences=True: pred, voted (T, M) int32 class ids,
    -1 none, -3 not evaluated.  One host synchronisation: the copy of the score table."""
    import torch
    cid = _ids_array(ids)
    k = int(cid.shape[0])
    vote = _check_vote(vote)
    emb = _device_embeddings(embeddings)
    m, dev = int(emb.shape[0]), emb.device
    slots = _expected_slots(expected, m, cid)
    rp = _rep_array(rep, m)
    pr = _prior_array(prior, k)
    train, evl, mix, minw, ok = _plan_table(plans)
    n_plans = len(train)
    masks = sorted({train[t] for t in range(n_plans) if ok[t]}) or [0]
    where = {mask: u for u, mask in enumerate(masks)}
    table = np.zeros(n_plans, dtype=_PLAN_DTYPE)
    for t in range(n_plans):                               # a plan the definition refuses reaches the device as one it refuses
        table[t] = (train[t], evl[t], where[train[t]], minw[t], mix[t]) if ok[t] else (0, 0, 0, 0, 0.0)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        slot_d, rep_d = torch.from_numpy(slots).to(dev), torch.from_numpy(rp).to(dev)
        prior_d = torch.from_numpy(pr).to(dev)
        masks_d = torch.from_numpy(np.array(masks, dtype=np.uint32).view(np.int32)).to(dev)
        plans_d = torch.from_numpy(table.view(np.uint8).reshape(n_plans, -1)).to(dev)
        sums = torch.empty(len(masks), MAX_CLASSES, ACC_W, dtype=torch.float64, device=dev)
        rows, unit = (torch.zeros(n_plans, k, D_E, dtype=torch.float32, device=dev) for _ in range(2))
        sc_d = torch.empty(n_plans, len(HOLDOUT_SCORE_KEYS), dtype=torch.int64, device=dev)
        conf = [torch.zeros(n_plans, MAX_CLASSES, MAX_CLASSES, dtype=torch.int32, device=dev) for _ in range(2)] if confusion else [None] * 2
        seq = [torch.full((n_plans, m), NOT_EVALUATED, dtype=torch.int32, device=dev) for _ in range(2)] if return_sequences else [None] * 2
        _lib.check(lib.cp_online_holdout_sums(emb.data_ptr(), m, k, slot_d.data_ptr(), rep_d.data_ptr(), masks_d.data_ptr(), len(masks),
                                              sums.data_ptr(), stream), "cp_online_holdout_sums")
        _lib.check(lib.cp_online_holdout_tables(sums.data_ptr(), len(masks), k, prior_d.data_ptr(), plans_d.data_ptr(), n_plans,
                                                rows.data_ptr(), unit.data_ptr(), stream), "cp_online_holdout_tables")
        _lib.check(lib.cp_online_holdout_score(emb.data_ptr(), m, k, slot_d.data_ptr(), rep_d.data_ptr(), unit.data_ptr(),
                                               plans_d.data_ptr(), n_plans, vote, sc_d.data_ptr(),
                                               *(None if x is None else x.data_ptr() for x in conf + seq), stream),
                   "cp_online_holdout_score")
        scores = sc_d.cpu().numpy()
        out = {key: scores[:, i].copy() for i, key in enumerate(HOLDOUT_SCORE_KEYS)}
        w = out["worst_class"]
        out["worst_class"] = np.where(w >= 0, cid[np.maximum(w, 0)], -1)           # slot -> class id
        out.update(rows=rows, unit=unit, sums=sums, sums_index=np.array(table["sums_index"], dtype=np.int64))
        if confusion:
            out.update(confusion=conf[0][:, :k, :k], voted_confusion=conf[1][:, :k, :k])
        if return_sequences:                               # slots -> class ids: -3, (-2), -1, ids
            to_id = torch.from_numpy(np.concatenate([[NOT_EVALUATED, IGNORE, -1], cid]).astype(np.int32)).to(dev)
            out.update(pred=to_id[(seq[0] + 3).long()], voted=to_id[(seq[1] + 3).long()])
    return out


def holdout_logits(embeddings, rows_or_unit, assign):
    """(M, K) f32 on the GPU: window i against the unit rows of plan assign[i] (cp_online_holdout_logits), NaN where assign[i]
    names no plan; `holdout_logits_reference` bit for bit.  rows_or_unit: what `score_plans` returned (its `unit` is read), or
    (T, K, 16) f32 unit rows on the GPU, taken as they are.  assign (M,) integers (`assign_folds`).  With every window
    assigned to the plan that held it out, the result serves as the `logits` of `thresholds_from_logits`, `sweep_gate`,
    `sweep_subsets` and `search_grasp_sets` as it is."""
    import torch
    unit = rows_or_unit["unit"] if isinstance(rows_or_unit, dict) else rows_or_unit
    emb = _device_embeddings(embeddings)
    m, dev = int(emb.shape[0]), emb.device
    if not isinstance(unit, torch.Tensor) or unit.dtype != torch.float32 or unit.dim() != 3 or unit.shape[2] != D_E \
            or unit.device != dev or not 1 <= unit.shape[0] <= MAX_PLANS or not 1 <= unit.shape[1] <= MAX_CLASSES:
        raise ValueError(f"unit rows must be a (T, K, 16) float32 tensor on the embeddings' device, T in 1..{MAX_PLANS}")
    a = np.asarray(_host(assign))
    if a.shape != (m,) or a.dtype.kind not in "iu":
        raise ValueError(f"assign must hold one integer entry per window ({m})")
    a = np.clip(a.astype(np.int64), -1, MAX_PLANS).astype(np.int32)
    n_plans, k = int(unit.shape[0]), int(unit.shape[1])
    lib = _lib.load()
    with torch.cuda.device(dev):
        unit = unit.contiguous()
        a_d = torch.from_numpy(a).to(dev)
        logits = torch.empty(m, k, dtype=torch.float32, device=dev)
        _lib.check(lib.cp_online_holdout_logits(emb.data_ptr(), m, k, unit.data_ptr(), n_plans, a_d.data_ptr(), logits.data_ptr(), k,
                                                torch.cuda.current_stream(dev).cuda_stream), "cp_online_holdout_logits")
    return logits


def _state_bytes(decoder, multi: bool) -> int:
    """the bytes at the start of a decoder's workspace that a push changes: stream states, and the adaptive forms' statistics"""
    a256 = lambda n: (n + 255) // 256 * 256
    s = decoder.n_streams if multi else 1
    adaptive = hasattr(decoder, "set_alpha") if multi else decoder.adapt is not None
    n = a256(s * _OL_STATE_BYTES) + (a256(s * _OLM_META_BYTES) if multi else 0)
    if adaptive:
        n += a256(s * _OLA_HEAD_BYTES) + a256(s * _OLA_STATS_BYTES)
    return n


def score_enrolment(decoder, raw, expected, plan="leave_one_out", stream: Optional[int] = None, folds: Optional[int] = None,
                    mix: float = 1.0, min_windows: int = 25, vote: Optional[int] = None) -> dict:
    """How well would rows enrolled from this cued recording decode a repetition they have not seen?  decoder: any of the four
    online decoders (a multi-stream one with `stream`), with a class table; raw (n, 12) f32 on the GPU; expected (M,) per
    window (`online.expected_commands`, `realign.realign_cues`).  plan: "leave_one_out", "learning_curve" or a plan list.
    The recording is embedded once (`track.embed_recording`), its repetitions come from `repetitions(expected, folds)`, the
    prior is the decoder's current class table and the ids its class ids; vote defaults to the decoder's.  The decoder is left
    as it was: stream state, vote ring, sample count, statistics and class table are put back.

    Returns what `score_plans` returns (one host synchronisation) and: plans; embeddings (M, 16) f32 on the GPU; rep (M,) and
    n_rep; assign (M,), for every
    window the plan that held its repetition out with the most training repetitions; logits (M, K) f32 on the GPU, the
    held-out logits under `assign`, for the gate and grasp-set sweeps; curve, {number of training repetitions: (summed
    voted_hit, summed n_cue)} over the plans, exact integers."""
    multi = isinstance(decoder.class_ids, (list, tuple))
    if multi and stream is None:
        raise ValueError("score_enrolment(decoder, raw, expected, stream=) on a multi-stream decoder")
    ids_t = decoder.class_ids[stream] if multi else decoder.class_ids
    if ids_t is None:
        raise _lib.CpNativeError("score_enrolment needs a class table: set_classes() first (it is the prior and the id list)")
    cid = _ids_array(ids_t)
    prior = (decoder.class_table(stream) if multi else decoder.class_table())[0]
    vote = _check_vote(decoder.vote if vote is None else vote)
    rep, n_rep = repetitions(expected, folds)
    if n_rep == 0:
        raise ValueError("the recording has no cued segment")
    if isinstance(plan, str):
        if plan not in ("leave_one_out", "learning_curve"):
            raise ValueError('plan must be "leave_one_out", "learning_curve" or a list of plans')
        plans = (leave_one_out if plan == "leave_one_out" else learning_curve)(n_rep, mix, min_windows)
    else:
        plans = list(plan)
    train, _, _, _, ok = _plan_table(plans)
    _expected_slots(expected, int(rep.shape[0]), cid)
    from .online import windows_before
    if raw.dim() != 2 or windows_before(int(raw.shape[0]), decoder.phase) != int(rep.shape[0]):
        raise ValueError("expected must hold one entry per window of the recording")
    # ---- the recording through the decoder's encoder, on a copy of what a push changes
    keep = decoder.ws[:_state_bytes(decoder, multi)].clone()
    seen = decoder._seen.copy() if multi else decoder.n_seen
    try:
        emb = embed_recording(decoder, raw, stream)
    finally:
        decoder.ws[:keep.numel()].copy_(keep)
        if multi:
            decoder._seen[:] = seen
        else:
            decoder.n_seen = seen
    out = score_plans(emb, expected, cid, rep, prior, plans, vote=vote)
    assign = assign_folds(rep, plans, most_trained=True)
    curve = {}
    for t in range(len(plans)):
        if ok[t] and out["n_cue"][t] >= 0:
            n = bin(train[t]).count("1")
            h, c = curve.get(n, (0, 0))
            curve[n] = (h + int(out["voted_hit"][t]), c + int(out["n_cue"][t]))
    out.update(plans=plans, rep=rep, n_rep=n_rep, assign=assign, logits=holdout_logits(emb, out, assign), embeddings=emb,
               curve=dict(sorted(curve.items())))
    return out
