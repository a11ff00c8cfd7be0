"""User metric: within-class whitening of the embedding on the GPU.

Every stage of the personalisation chain compares a window with a class row by a plain cosine in the 16-d space, which weighs
all sixteen directions alike.  A person's windows do not spread alike: contraction force, fatigue and arm position move every
grasp of a user along the same few directions, and a row that is right on average loses windows to a neighbour that lies along
such a loud axis.  The pooled within-class scatter (LDA) says which directions vary inside a grasp; whitening by it makes the
quiet directions that separate grasps count for more.  `fit_metric` finds a 16 x 16 lower-triangular A per user and shrink
value from a cued recording's embeddings (cp_online_metric_moments, cp_online_metric_factor, csrc/online_metric.cuh),
`Metric.apply` transforms a recording, `Metric.rows` fits class rows in the whitened space through the shipped centre-0 path,
and `MetricRows` is a stage behind any of the four decoders, as `PostureRows` is, that decodes the embeddings of every push
in that space (cp_online_metric_set / _reset / _push, one launch more per push).  `fit_reference`, `apply_reference` and
`stage_reference` are the definitions, in numpy with every operation rounded on its own (no fused multiply-add, no BLAS, no
np.linalg); the device equals them in every integer and bit (the payload of a NaN is not compared).

Moments.  embeddings e (M, 16) f32 as a push emits them; expected (M,) per window (class id, REST, IGNORE); ids (K,)
ascending, K <= 64; use (M,) bool, optional; min_windows >= 1.  A class's windows are those with its id, `use` set and 16
finite components, in window order.  Per class slot c, float64 accumulators from 0, one add per window in window order: the
count n_c, S_c[d] += float64(e[d]), P_c[i][j] += float64(e[i]) * float64(e[j]) for i <= j (136 entries, i-major; the product
of two f32 values is exact in float64, so only the add rounds).  `moments` holds S then P: (K, 152).

Scatter.  A class is fitted when n_c >= min_windows; C the fitted classes, N their windows.  N - C < 1: no metric.  For i <= j,
over the fitted classes in slot order: t = S_c[i] * S_c[j]; t = t / float64(n_c); Sw[i][j] += P_c[i][j] - t.  Then
Sw[i][j] /= float64(N - C).  tr = the diagonal summed in order, s = tr / 16; no metric unless s is finite and > 0.

Shrinkage and factor, per shrink value l in [0, 1] (up to 64 per call), all float64.  B[i][j] = (1 - l) * (Sw[i][j] / s) +
(l if i == j else 0.0) (the 0.0 is added: it turns a -0 into +0).  Cholesky B = L L^T row by row: r = B[i][j]; r = r - L[i][k] *
L[j][k] for k = 0..j-1; on the diagonal r is the pivot, and a pivot that is not > 0 or not finite means no metric for this l;
L[i][i] = sqrt(r), L[i][j] = r / L[j][j].  The inverse by forward substitution, column j by column j, rows in order:
Ai[j][j] = 1.0 / L[j][j]; for i > j: r = 0.0; r = r - L[i][k] * Ai[k][j] for k = j..i-1; Ai[i][j] = r / L[i][i].  A = float32(Ai),
lower triangular, +0 above the diagonal; an entry that is not finite in f32 means no metric for this l.  l = 1 gives the
identity in every bit.  Where there is no metric valid[t] = 0 and A[t] is the identity.

Apply, per window: y[i] = the f32 sum over j = 0..i, in that order, from 0, of A[i][j] * e[j]; ss = the f32 sum over i of
y[i] * y[i]; e'[i] = y[i] / sqrtf(ss), as the decoders' tail forms z / |z|.  A window with a component that is not finite (or
with y = 0) gives a row that is not finite.

Stage step, one window of one stream: e' as above; logit of slot k = the f32 sum over d = 0..15 of e'[d] * row[k][d], `row`
the stage's unit rows, normalised as `set_classes` normalises a table; if any of the K logits is not finite the window
predicts none (-1), otherwise the first maximum under `>` (-0 equals +0); the prediction enters the decoders' vote ring with
the decoder's ring length, where a none takes a place and does not vote; voted is the slot with the most entries, the
smallest among equals, none if no slot has one.  So `stage(e)` is the hold-out tail on `apply(e)`, and
`holdout.score_plans(apply(e), ...)` scores exactly what the stage will decode.

Nothing here is about real subjects; `metric_recording` is a synthetic person.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from . import holdout as H
from .holdout import _check_vote, _logits, _unit_rows, _vote_ring
from .prototypes import _int, _use_array
from .track import _expected_slots, _host, _ids_array

REST, IGNORE = -1, -2                   # online.REST, online.IGNORE
D_E = _lib.CP_D_E
MAX_CLASSES = _lib.CP_ONLINE_MAX_CLASSES
MAX_VOTE = _lib.CP_ONLINE_MAX_VOTE
MOMENTS = _lib.CP_ONLINE_METRIC_MOMENTS
MAX_SHRINKS = _lib.CP_ONLINE_METRIC_MAX_SHRINKS
VOTE = 25                               # online.VOTE
SHRINKS = (0.5, 0.2, 0.1, 0.05, 0.01)
_PI, _PJ = np.triu_indices(D_E)         # the 136 entries i <= j, i-major
_OM_WORDS = 4 + MAX_CLASSES + MAX_VOTE + D_E * D_E + MAX_CLASSES * D_E      # OmState in 32-bit words (csrc/online_metric.cuh; asserted in online_api.cuh)
assert MOMENTS == D_E + _PI.shape[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the definitions (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------
def _check_shrinks(shrink) -> np.ndarray:
    lam = np.asarray(_host(shrink), dtype=np.float64).reshape(-1)
    if not 1 <= lam.shape[0] <= MAX_SHRINKS:
        raise ValueError(f"1..{MAX_SHRINKS} shrink values, got {lam.shape[0]}")
    if not ((lam >= 0.0) & (lam <= 1.0)).all():
        raise ValueError("every shrink value must lie in [0, 1]")
    return lam


def _embeddings_array(embeddings) -> np.ndarray:
    emb = np.array(_host(embeddings), dtype=np.float32)
    if emb.ndim != 2 or emb.shape[1] != D_E:
        raise ValueError("embeddings must be (M, 16) float32")
    return emb


def moments_reference(embeddings, expected, ids, use=None):
    """The definition of the moments (module docstring): (moments (K, 152) f64, counts (K,) int64).  Host only (numpy)."""
    cid = _ids_array(ids)
    k = int(cid.shape[0])
    emb = _embeddings_array(embeddings)
    m = int(emb.shape[0])
    slots = _expected_slots(expected, m, cid).astype(np.int64)
    usev = _use_array(use, m)
    trains = np.isfinite(emb).all(axis=1) if usev is None else np.isfinite(emb).all(axis=1) & usev
    moments, counts = np.zeros((k, MOMENTS)), np.zeros(k, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(k):
            w = emb[trains & (slots == c)].astype(np.float64)
            counts[c] = w.shape[0]
            terms = np.concatenate([w, w[:, _PI] * w[:, _PJ]], axis=1)
            moments[c] = np.cumsum(np.concatenate([np.zeros((1, MOMENTS)), terms]), axis=0)[-1]    # (a cumulative sum is sequential)
    return moments, counts


def factor_reference(moments, counts, min_windows: int, shrink):
    """The definition of scatter, shrinkage and factor (module docstring): (A (T, 16, 16) f32, valid (T,) bool).  Host only."""
    lam = _check_shrinks(shrink)
    minw = _int(min_windows, "min_windows", 1, 2 ** 31 - 1)
    mom = np.asarray(moments, dtype=np.float64)
    cnt = np.asarray(counts, dtype=np.int64)
    if mom.ndim != 2 or mom.shape[1] != MOMENTS or cnt.shape != (mom.shape[0],):
        raise ValueError(f"moments (K, {MOMENTS}) and counts (K,)")
    n_t = int(lam.shape[0])
    out = np.tile(np.eye(D_E, dtype=np.float32), (n_t, 1, 1))
    valid = np.zeros(n_t, dtype=bool)
    fitted = np.nonzero(cnt >= minw)[0]
    n, c_fit = int(cnt[fitted].sum()), int(fitted.shape[0])
    if n - c_fit < 1:
        return out, valid
    with np.errstate(all="ignore"):
        sw = np.zeros(_PI.shape[0])
        for c in fitted.tolist():
            t = mom[c, _PI] * mom[c, _PJ]
            t = t / np.float64(cnt[c])
            sw = sw + (mom[c, D_E:] - t)
        sw = sw / np.float64(n - c_fit)
        full = np.zeros((D_E, D_E))
        full[_PI, _PJ] = sw
        full[_PJ, _PI] = sw
        tr = np.float64(0.0)
        for d in range(D_E):
            tr = tr + full[d, d]
        s = tr / np.float64(16.0)
        if not (np.isfinite(s) and s > 0):
            return out, valid
        for t in range(n_t):
            l = np.float64(lam[t])
            b = (np.float64(1.0) - l) * (full / s) + np.where(np.eye(D_E, dtype=bool), l, np.float64(0.0))
            low = np.zeros((D_E, D_E))
            ok = True
            for j in range(D_E):                               # column j of every row: each element's own k-sum is serial
                r = b[:, j].copy()
                for k in range(j):
                    r = r - low[:, k] * low[j, k]
                if not (r[j] > 0 and np.isfinite(r[j])):
                    ok = False
                    break
                low[j, j] = np.sqrt(r[j])
                low[j + 1:, j] = r[j + 1:] / low[j, j]
            if not ok:
                continue
            inv = np.zeros((D_E, D_E))
            for j in range(D_E):
                inv[j, j] = np.float64(1.0) / low[j, j]
                for i in range(j + 1, D_E):
                    r = np.float64(0.0)
                    for k in range(j, i):
                        r = r - low[i, k] * inv[k, j]
                    inv[i, j] = r / low[i, i]
            a32 = inv.astype(np.float32)
            if np.isfinite(a32).all():
                out[t], valid[t] = a32, True
    return out, valid


def fit_reference(embeddings, expected, ids, shrink=SHRINKS, min_windows: int = 25, use=None) -> dict:
    """The definition of the fit (module docstring).  embeddings (M, 16) f32; expected (M,) class ids, REST or IGNORE; ids the K
    ascending class ids; shrink one value or up to 64 in [0, 1]; min_windows >= 1; use (M,) bool or None.  Returns a dict:
    A (T, 16, 16) f32, valid (T,) bool, moments (K, 152) f64, counts (K,) int64, and ids, shrinks, min_windows as they were
    given.  Host only (numpy)."""
    lam = _check_shrinks(shrink)
    minw = _int(min_windows, "min_windows", 1, 2 ** 31 - 1)
    moments, counts = moments_reference(embeddings, expected, ids, use)
    a, valid = factor_reference(moments, counts, minw, lam)
    return dict(A=a, valid=valid, moments=moments, counts=counts, ids=_ids_array(ids), shrinks=lam, min_windows=minw)


def _matrix(a) -> np.ndarray:
    a32 = np.array(_host(a), dtype=np.float32)
    if a32.shape != (D_E, D_E):
        raise ValueError("A must be (16, 16) float32")
    return a32


def apply_reference(embeddings, a) -> np.ndarray:
    """The definition of the transform (module docstring): embeddings (M, 16) f32 and A (16, 16) f32, of which the lower
    triangle is read -> (M, 16) f32.  Host only (numpy)."""
    emb, a32 = _embeddings_array(embeddings), _matrix(a)
    m = int(emb.shape[0])
    y = np.zeros((m, D_E), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(D_E):
            s = np.zeros(m, dtype=np.float32)
            for j in range(i + 1):
                s = s + a32[i, j] * emb[:, j]
            y[:, i] = s
        ss = np.zeros(m, dtype=np.float32)
        for i in range(D_E):
            ss = ss + y[:, i] * y[:, i]
        return y / np.sqrt(ss)[:, None]


def _rows_array(rows, k: int) -> np.ndarray:
    r = np.array(_host(rows), dtype=np.float32)
    if r.shape != (k, D_E):
        raise ValueError(f"rows must hold one row of 16 per id ({k})")
    return r


def stage_reference(embeddings, a, rows, ids, vote: int = VOTE) -> dict:
    """The definition of the stage (module docstring) over one stream from an empty ring: embeddings (M, 16) f32 as a push
    emits them, A (16, 16) f32, rows (K, 16) f32 (normalised here as `set_classes` normalises a table), ids (K,) ascending.
    Returns a dict: pred, voted (M,) int64 class ids, -1 none; logits (M, K) f32; embeddings (M, 16) f32, the whitened unit
    embeddings.  Host only (numpy)."""
    cid = _ids_array(ids)
    k = int(cid.shape[0])
    vote = _check_vote(vote)
    e2 = apply_reference(embeddings, a)
    with np.errstate(all="ignore"):
        l = _logits(e2, _unit_rows(_rows_array(rows, k)))
        k1 = np.where(np.isfinite(l).all(axis=1), np.argmax(np.where(np.isnan(l), -np.inf, l), axis=1), -1) if l.shape[0] \
            else np.zeros(0, dtype=np.int64)
    voted = _vote_ring(k1, k, vote)
    to_id = np.concatenate([cid, [-1]])
    return dict(pred=to_id[k1], voted=to_id[voted], logits=l, embeddings=e2)


def metric_recording(m: int, k: int, seed: int = 0, segment: int = 40, rest: int = 10, loud: float = 0.6, quiet: float = 0.05,
                     spread: float = 0.3):
    """A synthetic cued recording of a person whose windows vary along one loud axis shared by all grasps, for tests and
    measurements; nothing about real subjects.  Returns (embeddings (m, 16) f32 unit rows, expected (m,) int64 class ids
    0..k-1 or REST).  The cue walks through the k classes again and again, `segment` windows per cue with `rest` REST windows
    behind each (noise alone).  a is a random unit vector, the loud axis; every class centre is one common unit vector b
    orthogonal to a plus `spread` times a unit vector of its own orthogonal to a and b.  A cued window is its centre plus
    `loud` * (g_r + g) * a, with g_r a standard normal number drawn once per cued segment (the force of that repetition) and g
    one per window, plus `quiet` * a standard normal vector; normalised.  Host only; the same arrays for the same arguments."""
    m, k = _int(m, "m", 1, 2 ** 31 - 1), _int(k, "k", 1, MAX_CLASSES)
    segment, rest = _int(segment, "segment", 1, 2 ** 31 - 1), _int(rest, "rest", 0, 2 ** 31 - 1)
    rng = np.random.default_rng(seed)
    unitv = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    a = unitv(rng.standard_normal(D_E))
    b = rng.standard_normal(D_E)
    b = unitv(b - (b @ a) * a)
    own = rng.standard_normal((k, D_E))
    own = own - (own @ a)[:, None] * a - (own @ b)[:, None] * b
    centres = b + spread * unitv(own)
    emb = np.zeros((m, D_E))
    exp = np.full(m, REST, dtype=np.int64)
    at = 0
    while at < m:
        for c in range(k):
            n = min(segment, m - at)
            force = rng.standard_normal()
            g = loud * (force + rng.standard_normal(n))
            emb[at:at + n] = unitv(centres[c] + g[:, None] * a + quiet * rng.standard_normal((n, D_E)))
            exp[at:at + n] = c
            at += n
            n = min(rest, m - at)
            emb[at:at + n] = unitv(rng.standard_normal((n, D_E)))
            at += n
            if at >= m:
                break
    return emb.astype(np.float32), exp


def _default_prior(k: int) -> np.ndarray:
    return np.full((k, D_E), 0.25, dtype=np.float32)          # a unit row; with mix = 1 only a class that is not enrolled keeps it


def _pick(fit, apply, score, embeddings, expected, ids, shrinks, folds, vote, min_windows, prior) -> dict:
    """`pick_shrink` over three callables: fit(use) -> (A, valid), apply(A[t]) -> embeddings, score(embeddings, plans) ->
    (voted hits, cue windows) summed over the plans"""
    cid = _ids_array(ids)
    lam = _check_shrinks(shrinks)
    vote = _check_vote(vote)
    minw = _int(min_windows, "min_windows", 1, 2 ** 31 - 1)
    rep, n_rep = H.repetitions(expected, folds)
    if n_rep < 2:
        raise ValueError("pick_shrink needs at least two repetitions of a cue")
    pr = _default_prior(int(cid.shape[0])) if prior is None else H._prior_array(prior, int(cid.shape[0]))
    plans = H.leave_one_out(n_rep, 1.0, minw)
    n_t = int(lam.shape[0])
    hits, cues, ok = np.zeros(n_t, dtype=np.int64), np.zeros(n_t, dtype=np.int64), np.ones(n_t, dtype=bool)
    base_hit = base_cue = 0
    for h in range(n_rep):
        bh, bc = score(embeddings, rep, pr, [plans[h]], vote)
        base_hit, base_cue = base_hit + bh, base_cue + bc
        a, valid = fit(rep != h, lam, minw)
        for t in range(n_t):
            if not valid[t]:
                ok[t] = False
                continue
            th, tc = score(apply(a[t]), rep, pr, [plans[h]], vote)
            hits[t], cues[t] = hits[t] + th, cues[t] + tc
    hits[~ok], cues[~ok] = -1, base_cue
    best = None
    for t in range(n_t):                                       # the most voted hits, the larger shrink value among equals
        if ok[t] and (best is None or (hits[t], lam[t]) > (hits[best], lam[best])):
            best = t
    return dict(shrinks=lam, voted_hit=hits, n_cue=cues, baseline=(int(base_hit), int(base_cue)), best=best,
                shrink=None if best is None else float(lam[best]), n_rep=n_rep)


def pick_shrink_reference(embeddings, expected, ids, shrinks=SHRINKS, folds: Optional[int] = None, vote: int = VOTE,
                          min_windows: int = 25, prior=None) -> dict:
    """`pick_shrink` on the definitions alone (`fit_reference`, `apply_reference`, `holdout.holdout_reference`).  Host only."""
    emb = _embeddings_array(embeddings)

    def score(e, rep, pr, plans, v):
        out = H.holdout_reference(e, expected, ids, rep, pr, plans, vote=v)
        return int(out["voted_hit"].sum()), int(out["n_cue"].sum())

    def fit(use, lam, minw):
        f = fit_reference(emb, expected, ids, lam, minw, use)
        return f["A"], f["valid"]

    return _pick(fit, lambda a: apply_reference(emb, a), score, emb, expected, ids, shrinks, folds, vote, min_windows, prior)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
class Metric:
    """What a fit found: ids (K,) int64; A (T, 16, 16) f32; valid (T,) bool, counts (K,) int64 and shrinks (T,) f64 as numpy;
    moments (K, 152) f64; min_windows as the fit took it.  A and moments are on the GPU after `fit_metric` and numpy after
    `Metric.of(fit_reference(...))`."""

    def __init__(self, ids, A, valid, counts, shrinks, min_windows, moments=None):
        self.ids = _ids_array(ids)
        self.A, self.moments = A, moments
        self.valid = np.asarray(valid).astype(bool).reshape(-1)
        self.counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        self.shrinks = np.asarray(shrinks, dtype=np.float64).reshape(-1)
        self.min_windows = int(min_windows)

    @classmethod
    def of(cls, fit: dict) -> "Metric":
        """A `Metric` from what `fit_reference` returned."""
        return cls(*(fit[key] for key in ("ids", "A", "valid", "counts", "shrinks", "min_windows", "moments")))

    def _t(self, t) -> int:
        n = int(self.valid.shape[0])
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) < n:
            raise IndexError(f"t must be an int in 0..{n - 1}, got {t!r}")
        if not self.valid[int(t)]:
            raise ValueError(f"shrink value {float(self.shrinks[int(t)])!r} gave no valid metric (too few windows, or a scatter that "
                             "does not factor)")
        return int(t)

    def apply(self, embeddings, t: int = 0):
        """The whitened unit embeddings (M, 16) f32 of embeddings (M, 16) f32 under A[t] (cp_online_metric_apply; with a numpy
        metric and numpy embeddings `apply_reference`).  A shrink value without a valid metric is a ValueError."""
        t = self._t(t)
        if isinstance(self.A, np.ndarray) and not hasattr(embeddings, "detach"):
            return apply_reference(embeddings, self.A[t])
        import torch
        emb = H._device_embeddings(embeddings)
        m, dev = int(emb.shape[0]), emb.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            a = torch.as_tensor(self.A[t]).to(device=dev, dtype=torch.float32).contiguous()
            out = torch.empty_like(emb)
            _lib.check(lib.cp_online_metric_apply(emb.data_ptr(), m, a.data_ptr(), out.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "cp_online_metric_apply")
        return out

    def rows(self, embeddings, expected, t: int = 0, min_windows: Optional[int] = None, use=None):
        """The class rows in the whitened space: (rows (K, 16) f32 on the GPU, valid (K,) bool numpy).  They come from the
        shipped centre-0 path, `fit_prototypes(self.apply(embeddings, t), expected, ids, rows_per_class=1, iters=0)`: the unit
        vector of the float64 sum of a class's whitened windows, the row `enroll` writes for a zero prior at mix = 1.  A class
        with fewer than min_windows windows (default: the fit's) is not valid and its row is 0: leave it out of the stage."""
        from .prototypes import fit_prototypes
        p = fit_prototypes(self.apply(embeddings, t), expected, self.ids, rows_per_class=1, iters=0,
                           min_windows=self.min_windows if min_windows is None else min_windows, use=use)
        return p.rows[:, 0].contiguous(), p.valid[:, 0].copy()

    def install(self, decoder, rows, ids=None, t: int = 0, stream: Optional[int] = None, stage: Optional["MetricRows"] = None) -> "MetricRows":
        """The stage for `decoder` (any of the four online decoders; a multi-stream one with `stream`) with A[t] and `rows`
        (K', 16) f32 under `ids` (default: the metric's).  Without stage= a new `MetricRows` is returned; stage=: an existing
        stage of this decoder, whose metric and rows of that stream are replaced and which is returned.  The decoder itself is
        not changed: its own table, pred and voted stay the plain-cosine ones."""
        if stage is None:
            return MetricRows(decoder, self, rows, ids, t, stream)
        if stage.decoder is not decoder:
            raise ValueError("stage= must be a MetricRows of this decoder")
        stage.set(self, rows, ids, t, stream)
        return stage


def fit_metric(embeddings, expected, ids, shrink=SHRINKS, min_windows: int = 25, use=None) -> Metric:
    """`fit_reference` on the device in two launches (cp_online_metric_moments: one wave per class; cp_online_metric_factor:
    one wave per shrink value).  embeddings (M, 16) f32 on the GPU (`track.embed_recording`); the other arguments as
    `fit_reference` takes them, checked before the first launch.  Returns a `Metric` whose A (T, 16, 16) f32 and moments
    (K, 152) f64 stay on the GPU and whose valid and counts are numpy, equal to the definition's.  One host synchronisation:
    the copy of those two."""
    import torch
    lam = _check_shrinks(shrink)
    minw = _int(min_windows, "min_windows", 1, 2 ** 31 - 1)
    cid = _ids_array(ids)
    k, n_t = int(cid.shape[0]), int(lam.shape[0])
    emb = H._device_embeddings(embeddings)
    m, dev = int(emb.shape[0]), emb.device
    slots = _expected_slots(expected, m, cid)
    usev = _use_array(use, m)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        slot_d = torch.from_numpy(slots).to(dev)
        use_d = None if usev is None else torch.from_numpy(usev.astype(np.uint8)).to(dev)
        moments = torch.empty(k, MOMENTS, dtype=torch.float64, device=dev)
        counts_d = torch.empty(k, dtype=torch.int64, device=dev)
        a = torch.empty(n_t, D_E, D_E, dtype=torch.float32, device=dev)
        valid_d = torch.empty(n_t, dtype=torch.uint8, device=dev)
        _lib.check(lib.cp_online_metric_moments(emb.data_ptr(), m, k, slot_d.data_ptr(), None if use_d is None else use_d.data_ptr(),
                                                moments.data_ptr(), counts_d.data_ptr(), stream), "cp_online_metric_moments")
        _lib.check(lib.cp_online_metric_factor(moments.data_ptr(), counts_d.data_ptr(), k, minw, (C.c_double * n_t)(*lam.tolist()), n_t,
                                               a.data_ptr(), valid_d.data_ptr(), stream), "cp_online_metric_factor")
        host = torch.cat([counts_d, valid_d.to(torch.int64)]).cpu().numpy()
    return Metric(cid, a, host[k:] != 0, host[:k], lam, minw, moments)


class MetricRows:
    """Decoding in a user's whitened space, behind any of the four decoders: per stream one state machine on the device that
    reads the embeddings of every push (include/cpnative.h, cp_online_metric_*; one launch more per push for any stream count,
    nothing is copied to the host).  The module docstring has the definition.

    source: any of the four online decoders.  metric, rows, ids, t: the `Metric`, whose A[t] is used, and the class rows
    (K, 16) f32 of the whitened space (`Metric.rows`) under the ascending ids (default: the metric's); on a multi-stream
    decoder they belong to `stream`, and further streams get theirs through `set` or `Metric.install(..., stage=)`.  A stream
    without a metric sits out: the stage hands on the decoder's own outputs for it.  A shrink value without a valid metric is a
    ValueError.

    The stage exposes what `CommandGate` and `GraspDrive` ask of a decoder -- `class_ids`, `n_seen`, `vote`, `push`,
    `push_packed`, `reset`, `device` -- so they stack on it unchanged: `CommandGate(stage)`, `GraspDrive(stage)`.  `push`
    returns the decoder's tuple shape, (pred, voted[, logits][, windows]), with pred and voted -1 for none and logits (M, K)
    against the stage's rows: the layout `thresholds_from_logits`, `sweep_gate`, `sweep_subsets`, `search_grasp_sets` and
    `CommandGate.apply` take, with `class_ids` as their ids.  It asks the decoder for the embeddings itself.

    The stage follows the decoder: a push or reset of the decoder behind its back makes the next `push` raise `CpNativeError`
    before anything is enqueued.  Its rows are its own: `set_classes`, `enroll` or `finetune` on the decoder do not reach
    them."""

    def __init__(self, source, metric: Optional[Metric] = None, rows=None, ids=None, t: int = 0, stream: Optional[int] = None):
        for name in ("class_ids", "n_seen", "vote", "push", "ws"):
            if not hasattr(source, name):
                raise TypeError("MetricRows wraps an OnlineDecoder, MultiStreamDecoder or AdaptiveMultiStreamDecoder")
        self.decoder = source
        self.multi = isinstance(source.class_ids, (list, tuple))
        self.n_streams = len(source.class_ids) if self.multi else 1
        self.vote = _int(source.vote, "vote", 1, MAX_VOTE)
        self.device = source.device
        self._ids = [None] * self.n_streams                 # the stage's class ids (K,) int64; None: the stream sits out
        self._pending = [None] * self.n_streams             # (A, rows, ids) set on the host, not yet on the device
        self.ws = None                                      # allocated with the first launch
        self._rows_cache = {}
        self._left = self._seen_now()
        if metric is not None:
            self.set(metric, rows, ids, t, stream)

    # ------------------------------------------------------------------ what a stage stacked on this one asks
    @property
    def n_seen(self):
        return self.decoder.n_seen

    @property
    def class_ids(self):
        """The class ids of the stage's rows, ascending: (K,) int64 numpy; for a stream that sits out the decoder's own; on a
        multi-stream decoder a list with one per stream."""
        if self.multi:
            return [self.decoder.class_ids[s] if i is None else i for s, i in enumerate(self._ids)]
        return self.decoder.class_ids if self._ids[0] is None else self._ids[0]

    def _index(self, stream) -> int:
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {stream!r}")
        return int(stream)

    def set(self, metric: Metric, rows, ids=None, t: int = 0, stream: Optional[int] = None):
        """The metric A[t] and the class rows (K, 16) f32 under `ids` (default: the metric's) of one stream.  They go in with
        the next launch; that stream's ring empties."""
        if self.multi and stream is None:
            raise ValueError("set(metric, rows, ids, t, stream) on a multi-stream decoder")
        s = self._index(stream) if self.multi else 0
        if not isinstance(metric, Metric):
            raise TypeError("metric must be a Metric (fit_metric, or Metric.of(fit_reference(...)))")
        t = metric._t(t)
        cid = _ids_array(metric.ids if ids is None else ids)
        if rows is None or tuple(rows.shape) != (int(cid.shape[0]), D_E):
            raise ValueError(f"rows must hold one row of 16 per id ({int(cid.shape[0])})")
        self._pending[s] = (metric.A[t], rows, cid)
        self._ids[s] = cid

    # ------------------------------------------------------------------ the device side (one method per C entry)
    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _args(self):
        if self.ws is None:
            import torch
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_metric_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return self.vote, self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_set(self, s: int, a, rows, ids: np.ndarray):
        import torch
        k = int(ids.shape[0])
        args = self._args()
        a_d = torch.as_tensor(a).to(device=self.device, dtype=torch.float32).contiguous()
        r_d = torch.as_tensor(rows).to(device=self.device, dtype=torch.float32).contiguous()
        _lib.check(self.lib.cp_online_metric_set(*args, s, a_d.data_ptr(), r_d.data_ptr(), (C.c_int32 * k)(*ids.tolist()), k,
                                                 self._stream()), "cp_online_metric_set")

    def _dev_reset(self, s: int):
        args = self._args()
        _lib.check(self.lib.cp_online_metric_reset(*args, s, _lib.CP_ONLINE_METRIC_RESET_RING, self._stream()), "cp_online_metric_reset")

    def _dev_push(self, emb, row0: np.ndarray, m: np.ndarray, rows: int, want_logits: bool):
        """one launch over `rows` packed rows -> (pred, voted) (2, rows) int32 and logits (rows, 64) f32 or None"""
        import torch
        from .online import _rows_on_device
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.device)
        pv = torch.empty(2, rows, dtype=torch.int32, device=self.device)
        logits = torch.empty(rows, MAX_CLASSES, dtype=torch.float32, device=self.device) if want_logits else None
        _lib.check(self.lib.cp_online_metric_push(*args, emb.data_ptr(), rm[0].data_ptr(), rm[1].data_ptr(), rows, pv[0].data_ptr(),
                                                  pv[1].data_ptr(), logits.data_ptr() if want_logits else None, MAX_CLASSES,
                                                  self._stream()), "cp_online_metric_push")
        return pv, logits

    # ------------------------------------------------------------------ staying in step with the decoder
    def _seen_now(self) -> np.ndarray:
        return np.array(self.decoder.n_seen, dtype=np.int64).reshape(-1).copy()

    def _sync(self):
        for s in range(self.n_streams):
            if self._pending[s] is not None:
                self._dev_set(s, *self._pending[s])
                self._pending[s] = None

    def _check_in_step(self):
        if not np.array_equal(self._seen_now(), self._left):
            raise _lib.CpNativeError("the decoder was pushed or reset behind the metric stage (its n_seen is not what the stage "
                                     "left): the stage's ring no longer follows the stream; push and reset through the stage, or "
                                     "reset() it")

    # ------------------------------------------------------------------ the stage over per-stream embeddings
    def _stage(self, per_stream, want_logits: bool, strict: bool):
        """per_stream: n_streams entries, None or (M_s, 16) f32 embeddings -> per stream (pred, voted, logits or None), None
        for a stream that sits out (strict: embeddings for such a stream are refused)"""
        import torch
        self._sync()
        step = _lib.CP_ONLINE_MAX_WINDOWS
        ms = []
        for s, t in enumerate(per_stream):
            if t is None:
                ms.append(0)
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != D_E \
                    or t.device.type != "cuda":
                raise ValueError("embeddings must be (M, 16) float32 tensors on the GPU")
            if strict and t.shape[0] and self._ids[s] is None:
                raise _lib.CpNativeError(f"stream {s} has embeddings but no metric: set(metric, rows, ...) first")
            ms.append(int(t.shape[0]))
        live = np.array([i is not None for i in self._ids])
        outs = []
        for lo in range(0, max(max(ms), 1), step):
            n_all = np.array([min(max(n - lo, 0), step) for n in ms], dtype=np.int64)
            rows = int(n_all.sum())
            row0 = np.zeros_like(n_all)
            np.cumsum(n_all[:-1], out=row0[1:])
            m = np.where(live, n_all, 0)                       # a stream that sits out keeps its place in the packed rows
            if int(m.sum()) == 0:
                pv = torch.empty(2, rows, dtype=torch.int32, device=self.device)
                logits = torch.empty(rows, MAX_CLASSES, dtype=torch.float32, device=self.device) if want_logits else None
            else:
                views = [per_stream[s][lo:lo + n] for s, n in enumerate(n_all.tolist()) if n]
                base = views[0]
                packed = base.stride() == (D_E, 1) and base.data_ptr() % 16 == 0
                for v, r in zip(views, row0[n_all > 0].tolist()):   # the packed output of one push lies as the launch reads it
                    packed = packed and v.stride() == (D_E, 1) and v.data_ptr() == base.data_ptr() + 4 * D_E * r
                emb = base if packed else torch.cat(views).contiguous()
                pv, logits = self._dev_push(emb, row0, m, rows, want_logits)
            nl = n_all.tolist()
            lg = [None] * self.n_streams if logits is None else \
                [x[:, :(0 if i is None else i.shape[0])] for x, i in zip(logits.split(nl), self._ids)]
            outs.append(list(zip(pv[0].split(nl), pv[1].split(nl), lg)))
        if len(outs) == 1:
            res = outs[0]
        else:
            res = [tuple(None if outs[0][s][i] is None else torch.cat([o[s][i] for o in outs]) for i in range(3))
                   for s in range(self.n_streams)]
        return [r if i is not None else None for r, i in zip(res, self._ids)]

    # ------------------------------------------------------------------ API
    def apply(self, embeddings, return_logits: bool = False):
        """The stage alone on embeddings the caller already has (of the decoder's next windows, in order): (M, 16) f32 on the
        GPU -> (pred, voted[, logits]); on a multi-stream decoder a list with one entry per stream (None: no windows) -> one
        such tuple per stream (None for a stream that sits out).  pred, voted (M,) int32 class ids or -1, logits (M, K) f32."""
        import torch
        pick = lambda r: None if r is None else (r if return_logits else r[:2])
        if self.multi:
            if isinstance(embeddings, torch.Tensor) or len(embeddings) != self.n_streams:
                raise ValueError(f"embeddings must be a sequence of {self.n_streams} entries (None or (M, 16) tensors)")
            out = [pick(r) for r in self._stage(list(embeddings), return_logits, True)]
        else:
            out = pick(self._stage([embeddings], return_logits, True)[0])
        self._left = self._seen_now()
        return out

    def _passes(self) -> bool:
        return any(i is None for i in self._ids)

    @staticmethod
    def _pick(res, staged, own_logits: bool, return_logits: bool, return_windows: bool):
        """res: the decoder's (pred, voted[, logits][, windows], embeddings); staged: (pred, voted, logits) or None"""
        at = 2 + int(own_logits)
        if staged is None:
            out = [res[0], res[1]] + ([res[2]] if return_logits else [])
        else:
            out = [staged[0], staged[1]] + ([staged[2]] if return_logits else [])
        if return_windows:
            out.append(res[at])
        return tuple(out)

    def push(self, raw, return_logits: bool = False, return_windows: bool = False):
        """What the decoder's `push` takes (raw (n, 12), or one chunk per stream) -> (pred, voted[, logits][, windows]) per
        stream, decoded in the stream's whitened space; for a stream that sits out the decoder's own."""
        self._check_in_step()
        self._sync()
        own = return_logits and self._passes()
        res = self.decoder.push(raw, return_logits=own, return_windows=return_windows, return_embeddings=True)
        return self._finish(res, own, return_logits, return_windows)

    def push_packed(self, raw, counts, return_logits: bool = False, return_windows: bool = False):
        """`push` for samples packed in stream order, as the multi-stream decoders' `push_packed`."""
        if not self.multi:
            raise TypeError("push_packed belongs to the multi-stream decoders")
        self._check_in_step()
        self._sync()
        own = return_logits and self._passes()
        res = self.decoder.push_packed(raw, counts, return_logits=own, return_windows=return_windows, return_embeddings=True)
        return self._finish(res, own, return_logits, return_windows)

    def _finish(self, res, own: bool, return_logits: bool, return_windows: bool):
        self._left = self._seen_now()
        if self.multi:
            staged = self._stage([r[-1] for r in res], return_logits, False)
            return [self._pick(r, t, own, return_logits, return_windows) for r, t in zip(res, staged)]
        return self._pick(res, self._stage([res[-1]], return_logits, False)[0], own, return_logits, return_windows)

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back (this waits for the device; a test and debugging aid): ids,
        has_metric, A (16, 16) f32, rows (K, 16) f32 (the unit rows), and ring, the slots (-1: none) from the oldest to the
        newest.  The layout is that of OmState (csrc/online_metric.cuh): int32 K, has_metric, head, len, ids[64], ring[256];
        f32 A[256], row[64][16]."""
        import torch
        s = self._index(stream)
        self._sync()
        if self.ws is None:
            return dict(ids=[], has_metric=0, A=np.zeros((D_E, D_E), np.float32), rows=np.zeros((0, D_E), np.float32), ring=[])
        w = self.ws[:self.n_streams * _OM_WORDS * 4].view(torch.int32).reshape(self.n_streams, _OM_WORDS)[s].cpu().numpy()
        k, has, head, n = (int(x) for x in w[:4])
        ring = w[4 + MAX_CLASSES:4 + MAX_CLASSES + MAX_VOTE]
        f = w[4 + MAX_CLASSES + MAX_VOTE:].view(np.float32)
        return dict(ids=w[4:4 + k].tolist(), has_metric=has, A=f[:D_E * D_E].reshape(D_E, D_E).copy(),
                    rows=f[D_E * D_E:].reshape(MAX_CLASSES, D_E)[:k].copy(),
                    ring=[int(ring[(head - n + i) % self.vote]) for i in range(n)])

    def reset(self, streams=None):
        """Reset the decoder and the stage's ring (metric and rows stay); on a multi-stream decoder the listed streams,
        default all."""
        self._sync()
        if self.multi and streams is not None:
            idx = sorted({self._index(s) for s in streams})
            self.decoder.reset(idx)
            for s in idx:
                self._dev_reset(s)
        else:
            self.decoder.reset()
            self._dev_reset(-1)
        self._left = self._seen_now()


def pick_shrink(embeddings, expected, ids, shrinks=SHRINKS, folds: Optional[int] = None, vote: int = VOTE, min_windows: int = 25,
                prior=None) -> dict:
    """Which shrink value decodes repetitions it has not seen best?  Host glue over device calls.  embeddings (M, 16) f32 on
    the GPU; expected (M,) per window; ids the K ascending class ids; shrinks 1..64 values in [0, 1].  Per repetition h of
    `holdout.repetitions(expected, folds)`: `fit_metric` on the other repetitions through `use=`, `Metric.apply` to the whole
    recording per shrink value, and `holdout.score_plans` with plan h of `holdout.leave_one_out` (mix 1: the rows are enrolled
    in the whitened space from the training repetitions; prior: the rows of classes that are not enrolled, default a constant
    unit row).  Returns a dict: shrinks (T,) f64; voted_hit, n_cue (T,) int64, the voted hits and cue windows summed over the
    held-out repetitions, exact integers (-1 hits for a shrink value that gave no valid metric in some fold); baseline, the
    same pair from the untransformed embeddings (the plain cosine); best, the index with the most voted hits, the larger shrink
    value among equals (None if none is valid); shrink, its value; n_rep."""
    emb = H._device_embeddings(embeddings)

    def score(e, rep, pr, plans, v):
        out = H.score_plans(e, expected, ids, rep, pr, plans, vote=v)
        return int(out["voted_hit"].sum()), int(out["n_cue"].sum())

    box = {}

    def fit(use, lam, minw):
        box["m"] = fit_metric(emb, expected, ids, lam, minw, use)
        return list(range(int(lam.shape[0]))), box["m"].valid

    return _pick(fit, lambda t: box["m"].apply(emb, t), score, emb, expected, ids, shrinks, folds, vote, min_windows, prior)


def metric_enrolment(decoder, raw, expected, shrinks=SHRINKS, stream: Optional[int] = None, folds: Optional[int] = None,
                     min_windows: int = 25, vote: Optional[int] = None, ids=None, stage: Optional[MetricRows] = None) -> dict:
    """The whole chain for one user: `track.embed_recording` -> `pick_shrink` -> `fit_metric` on everything with the picked
    shrink value -> `Metric.rows` -> the installed stage.  decoder: any of the four online decoders (a multi-stream one with
    `stream`); raw (n, 12) f32 on the GPU; expected (M,) per window; ids: the class ids (default: the decoder's).  The decoder
    is left as it was, as `score_enrolment` leaves it: stream state, vote ring, sample count and statistics are put back.  Only
    the classes whose row is valid enter the stage.  Returns a dict: stage (`MetricRows`), metric (`Metric`, one shrink value),
    shrink, pick (what `pick_shrink` returned), rows (K, 16) f32 on the GPU, valid (K,) bool, embeddings (M, 16) f32."""
    import torch
    multi = isinstance(decoder.class_ids, (list, tuple))
    if multi and stream is None:
        raise ValueError("metric_enrolment(decoder, raw, expected, stream=) on a multi-stream decoder")
    if ids is None:
        ids = decoder.class_ids[stream] if multi else decoder.class_ids
        if ids is None:
            raise _lib.CpNativeError("metric_enrolment needs class ids: set_classes() first, or ids=")
    cid = _ids_array(ids)
    lam = _check_shrinks(shrinks)
    vote = _check_vote(decoder.vote if vote is None else vote)
    keep = decoder.ws[:H._state_bytes(decoder, multi)].clone()
    seen = decoder._seen.copy() if multi else decoder.n_seen
    try:
        emb = H.embed_recording(decoder, raw, stream)
    finally:
        decoder.ws[:keep.numel()].copy_(keep)
        if multi:
            decoder._seen[:] = seen
        else:
            decoder.n_seen = seen
    pick = pick_shrink(emb, expected, cid, lam, folds, vote, min_windows)
    if pick["best"] is None:
        raise ValueError("no shrink value gave a valid metric in every fold")
    metric = fit_metric(emb, expected, cid, [pick["shrink"]], min_windows)
    rows, valid = metric.rows(emb, expected, 0, min_windows)
    if not valid.any():
        raise ValueError("no class has min_windows windows")
    on = torch.from_numpy(np.nonzero(valid)[0]).to(rows.device)
    st = metric.install(decoder, rows[on].contiguous(), cid[valid], 0, stream, stage)
    return dict(stage=st, metric=metric, shrink=pick["shrink"], pick=pick, rows=rows, valid=valid, embeddings=emb)
