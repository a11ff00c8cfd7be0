"""Cue realignment: the onset and offset of each cued movement, from the sEMG itself.

The model was trained on Ninapro's `restimulus`, labels whose starts and ends had been moved from the cue onto the activity
seen in the sEMG.  A user's own cued recording has no such relabelling: the person starts some hundred milliseconds after
the cue and lets go late, so the first part of every cued segment is rest labelled as a grasp and the start of every rest
period a grasp labelled as rest.  `realign_cues` produces the labels the personalisation chain was designed to receive, in
front of `enroll`, without the model, on the device on the windows `recording_windows` leaves there (cp_online_realign*,
csrc/online_realign.cuh).  `realign_reference` is the definition, in numpy and Python integers; the device equals it in every
integer.

Activity.  One integer per window: per channel d, v = (x_d - base_d) * gain_d as two float32 operations, r = rint(v) (ties to
even), q_d = 0 unless r > 0 (NaN lands here), 255 if r >= 255, else int(r); a[k] = sum_d q_d in 0..3060 (`activity_reference`).
A caller's own activity is clamped to 0..MAX_ACTIVITY.

Segments.  `cue_segments(cue)`: the maximal runs of consecutive windows with the same cue >= 0 (`score_commands`' segments), rows
[s, e) in ascending order.

Region of row i, with prev_e the e of the row before (0 for the first) and next_s the s of the row behind (M for the last):
r0 = max(s - context, prev_e), r1 = min(e + max_lag, next_s), L = r1 - r0, P the exclusive prefix sum of a over the region,
T = P[L].  (A table with bad rows, which `cue_segments` never makes: a row that is not 0 <= s < e <= M with prev_e <= s has
status 4; the bounds a good row takes from a bad neighbour are brought into range, r0 = max(s - context, prev_e, 0) and
r1 = min(e + max_lag, max(next_s, e), M).)

Candidates.  The pairs (o, f) with s <= o <= min(s + max_lag, e - min_len), max(o + min_len, e - max_lead) <= f <= r1,
n_A = f - o, n_R = L - n_A >= min_rest; S_A = sum a[o..f), S_R = T - S_A.  A pair has the contrast if
S_A n_R - S_R n_A >= max(min_contrast n_A n_R, 1): the active mean is above the resting mean, by min_contrast at least.

Choice.  The least-squares fit of two levels maximises p / q with p = S_A^2 n_R + S_R^2 n_A and q = n_A n_R; fractions are
compared exactly by cross-multiplication, equals go to the smaller o, then the smaller f.  With a <= 4095 and L <= 4096,
p <= 4095^2 n_A n_R L < 2^58 and q < 2^24: the products need 128 bits, and a comparison cut to 64 picks other pairs.

Status.  0: the best pair with the contrast.  1: no pair meets the length limits.  2: pairs exist, none has the contrast; the
best of them all is reported.  3: L > MAX_REGION.  4: a bad table row; nothing of that segment is read or written.

Labels, in the coding of `expected_commands` (class id, REST, IGNORE): out[k] = cue[k] where cue[k] < 0, else IGNORE; then for
a segment with status 0 and c = cue[s], over k in [s, r1): c if o + guard <= k < f - guard; else for k < e: REST if
k < o - guard or k >= f + guard, else IGNORE; else IGNORE if k < f + guard, else cue[k].  A segment with another status keeps
IGNORE over [s, e).  The ranges [s, r1) of different segments are disjoint (r1 of one is at most s of the next).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

REST, IGNORE = -1, -2                   # online.REST, online.IGNORE
STRIDE = _lib.CP_ONLINE_STRIDE
EMG_DIM = _lib.CP_EMG_DIM
MAX_ACTIVITY = _lib.CP_ONLINE_REALIGN_MAX_ACTIVITY
MAX_REGION = _lib.CP_ONLINE_REALIGN_MAX_REGION
MAX_SEGMENTS = 65536
FOUND, NO_PAIR, NO_CONTRAST, TOO_LONG, BAD_ROW = 0, 1, 2, 3, 4
SEGMENT_COLUMNS = ("start", "end", "onset", "offset", "status", "cls", "lag", "overrun")
_PARAMS = ("max_lag", "max_lead", "min_len", "min_rest", "context", "min_contrast", "guard")


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _check_params(p: dict) -> dict:
    out = {}
    for k in _PARAMS:
        v = p[k]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{k} must be an integer")
        out[k] = int(v)
    for k, top in (("max_lag", 1024), ("max_lead", 1024), ("context", 2048), ("min_contrast", MAX_ACTIVITY)):
        if not 0 <= out[k] <= top:
            raise ValueError(f"{k} must lie in 0..{top}")
    for k in ("min_len", "min_rest"):
        if not 1 <= out[k] < 2 ** 31:
            raise ValueError(f"{k} must be at least 1")
    if out["guard"] < 0 or out["min_len"] <= 2 * out["guard"]:
        raise ValueError("guard must not be negative, and min_len must exceed 2 guard")
    return out


def _cue_array(cue) -> np.ndarray:
    c = _host(cue)
    if c.ndim != 1 or c.dtype.kind not in "iu":
        raise ValueError("cue must be a 1-d integer array: a class id, REST or IGNORE per window")
    c = c.astype(np.int64)
    if c.shape[0] and (c.min() < -2 ** 31 or c.max() >= 2 ** 31):
        raise ValueError("cue must fit 32 bits")
    return c


def _activity_array(activity, m: int) -> np.ndarray:
    a = _host(activity)
    if a.ndim != 1 or a.dtype.kind not in "iu" or a.shape[0] != m:
        raise ValueError(f"activity must be a 1-d integer array with one entry per window ({m})")
    return np.clip(a.astype(np.int64), 0, MAX_ACTIVITY)


def cue_segments(cue) -> np.ndarray:
    """The cued segments of `cue` (M,): the maximal runs of consecutive windows with the same cue >= 0, as (n_seg, 2) int32 rows
    [s, e) in ascending order.  Host only (numpy)."""
    c = _cue_array(cue)
    on = c >= 0
    start = np.nonzero(on & (c != np.concatenate([[IGNORE], c[:-1]])))[0]
    end = np.nonzero(on & (c != np.concatenate([c[1:], [IGNORE]])))[0] + 1
    return np.stack([start, end], axis=1).astype(np.int32)


def activity_reference(windows, base, gain) -> np.ndarray:
    """The activity of each window of `windows` (M, 12) under base and gain (12,) each: (M,) int32.  numpy float32, operation
    for operation what the device does.  Host only."""
    x = np.asarray(_host(windows), dtype=np.float32)
    b = np.asarray(_host(base), dtype=np.float32).reshape(-1)
    g = np.asarray(_host(gain), dtype=np.float32).reshape(-1)
    if x.ndim != 2 or x.shape[1] != EMG_DIM or b.shape[0] != EMG_DIM or g.shape[0] != EMG_DIM:
        raise ValueError(f"windows (M, {EMG_DIM}), base ({EMG_DIM},) and gain ({EMG_DIM},) go together")
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - b[None, :]
        r = np.rint(d * g[None, :])
        q = np.where(r > 0, np.minimum(r, np.float32(255)), np.float32(0))
    return q.astype(np.int64).sum(axis=1).astype(np.int32)


def _before(a, b) -> bool:
    """the order of the choice on (flag, p, q, o, f) in Python integers: a before b"""
    if a[0] != b[0]:
        return a[0] > b[0]
    lhs, rhs = a[1] * b[2], b[1] * a[2]
    if lhs != rhs:
        return lhs > rhs
    return (a[3], a[4]) < (b[3], b[4])


def _choose(P: np.ndarray, so: int, eo: int, L: int, c: dict):
    """The choice among the pairs of one region, o and f counted from r0: (flag, p, q, o, f) or None.  Each onset's pairs are
    formed in int64 (exact: p < 2^58); a float64 quotient, good to a few units in 2^-53, only drops pairs that lie 2^-40 below
    the onset's largest, and what is left is compared in Python integers."""
    T = int(P[L])
    short = []
    for o in range(so, min(so + c["max_lag"], eo - c["min_len"]) + 1):
        f = np.arange(max(o + c["min_len"], eo - c["max_lead"]), min(L, o + L - c["min_rest"]) + 1, dtype=np.int64)
        if f.shape[0] == 0:
            continue
        nA = f - o
        nR = L - nA
        SA = P[f] - P[o]
        SR = T - SA
        q = nA * nR
        p = SA * SA * nR + SR * SR * nA
        flag = SA * nR - SR * nA >= np.maximum(c["min_contrast"] * q, 1)
        for want in (True, False):
            idx = np.nonzero(flag == want)[0]
            if idx.shape[0]:
                g = p[idx] / q[idx]
                keep = idx[g >= g.max() * (1.0 - 2.0 ** -40)]
                short += [(int(want), int(p[j]), int(q[j]), o, int(f[j])) for j in keep]
    best = None
    for cand in short:
        if best is None or _before(cand, best):
            best = cand
    return best


def realign_reference(activity, cue, segments, *, max_lag, max_lead, min_len, min_rest, context, min_contrast, guard):
    """The definition of cue realignment (see the module's docstring).  activity (M,) integers, cue (M,) integers, segments
    (n_seg, 2) integer rows [s, e).  Returns (expected (M,) int64, table (n_seg, 8) int32: s, e, r0, r1, onset, offset, status,
    cue[s], sums (n_seg, 2) int64: S_A, S_R of the reported pair).  Host only."""
    c = _check_params(dict(max_lag=max_lag, max_lead=max_lead, min_len=min_len, min_rest=min_rest, context=context,
                           min_contrast=min_contrast, guard=guard))
    cu = _cue_array(cue)
    M = cu.shape[0]
    a = _activity_array(activity, M)
    seg = np.asarray(_host(segments))
    if seg.ndim != 2 or seg.shape[1] != 2 or seg.dtype.kind not in "iu":
        raise ValueError("segments must be (n_seg, 2) integers")
    seg = seg.astype(np.int64)
    n = seg.shape[0]
    out = np.where(cu < 0, cu, IGNORE).astype(np.int64)
    table = np.zeros((n, 8), dtype=np.int32)
    sums = np.zeros((n, 2), dtype=np.int64)
    g = c["guard"]
    for i in range(n):
        s, e = int(seg[i, 0]), int(seg[i, 1])
        prev_e = int(seg[i - 1, 1]) if i > 0 else 0
        next_s = int(seg[i + 1, 0]) if i + 1 < n else M
        if not (0 <= s < e <= M and prev_e <= s):
            table[i] = (s, e, -1, -1, -1, -1, BAD_ROW, -1)
            continue
        r0 = max(s - c["context"], prev_e, 0)
        r1 = min(e + c["max_lag"], max(next_s, e), M)
        L = r1 - r0
        cls = int(cu[s])
        if L > MAX_REGION:
            table[i] = (s, e, r0, r1, -1, -1, TOO_LONG, cls)
            continue
        P = np.concatenate([[0], np.cumsum(a[r0:r1])]).astype(np.int64)
        best = _choose(P, s - r0, e - r0, L, c)
        if best is None:
            table[i] = (s, e, r0, r1, -1, -1, NO_PAIR, cls)
            continue
        o, f = r0 + best[3], r0 + best[4]
        SA = int(P[best[4]] - P[best[3]])
        sums[i] = (SA, int(P[L]) - SA)
        table[i] = (s, e, r0, r1, o, f, FOUND if best[0] else NO_CONTRAST, cls)
        if not best[0]:
            continue
        k = np.arange(s, r1)
        inside = (k >= o + g) & (k < f - g)
        clear = (k < o - g) | (k >= f + g)
        out[s:r1] = np.where(inside, cls, np.where(k < e, np.where(clear, REST, IGNORE), np.where(k < f + g, IGNORE, cu[s:r1])))
    return out, table, sums


# ---------------------------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------------------------
def activity_profile(windows, cue, level: float = 0.95, settle: int = 100) -> dict:
    """base and gain of the activity, from the recording itself: windows (M, 12), the normalised windows (`recording_windows`),
    and cue (M,) as `expected_commands` gives it.  Host only (numpy), as `drive_profile` is.  Returns dict(base, gain), (12,)
    float32 each:
      base   the per-channel median over the REST windows that lie at least `settle` windows behind the last window with
             cue >= 0 (the hand has let go by then), or over all REST windows if none does;
      gain   float32(255 / span) with span the `level` quantile over the windows with cue >= 0, minus base; 0 where the span
             is not positive and finite (the channel adds nothing).
    A recording without a REST window is refused."""
    w = np.asarray(_host(windows), dtype=np.float64)
    c = _cue_array(cue)
    if w.ndim != 2 or w.shape[1] != EMG_DIM or c.shape[0] != w.shape[0]:
        raise ValueError(f"windows (M, {EMG_DIM}) and cue (M,) go together")
    if not 0.0 < float(level) <= 1.0:
        raise ValueError("level must lie in (0, 1]")
    if isinstance(settle, bool) or not isinstance(settle, (int, np.integer)) or settle < 0:
        raise ValueError("settle must be a non-negative integer")
    rest = c == REST
    if not rest.any():
        raise ValueError("the recording has no REST windows: the resting level is taken from them")
    k = np.arange(c.shape[0])
    last_cue = np.maximum.accumulate(np.where(c >= 0, k, -1 - int(settle)))      # (before the first cue: far enough)
    settled = rest & (k - last_cue >= int(settle))
    base = np.median(w[settled if settled.any() else rest], axis=0)
    cued = w[c >= 0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        span = (np.quantile(cued, float(level), axis=0) if cued.shape[0] else np.zeros(EMG_DIM)) - base
        gain = np.where(np.isfinite(span) & (span > 0), 255.0 / np.where(span > 0, span, 1.0), 0.0).astype(np.float32)
    gain = np.where(np.isfinite(gain), gain, np.float32(0)).astype(np.float32)
    return dict(base=base.astype(np.float32), gain=gain)


def _check_profile(profile) -> tuple:
    try:
        base = np.asarray(_host(profile["base"]), dtype=np.float32).reshape(-1)
        gain = np.asarray(_host(profile["gain"]), dtype=np.float32).reshape(-1)
    except (KeyError, TypeError, IndexError):
        raise ValueError("profile must be a dict with base and gain, as activity_profile returns it") from None
    if base.shape[0] != EMG_DIM or gain.shape[0] != EMG_DIM:
        raise ValueError(f"profile: base and gain must hold {EMG_DIM} values each")
    return np.ascontiguousarray(base), np.ascontiguousarray(gain)


def _realign_dev(windows, activity, cue32: np.ndarray, segments: np.ndarray, cfg: dict, base, gain, device):
    """the device side of `realign_cues` (cp_online_realign_activity unless `activity` is given, then cp_online_realign) ->
    expected (M,) int32, table (n_seg, 8) int32, sums (n_seg, 2) int64 on the host, fetched in one copy"""
    import torch
    lib = _lib.load()
    m, n = int(cue32.shape[0]), int(segments.shape[0])
    if device is None:                                                   # a host activity and no windows: torch's current GPU
        device = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if activity is None:
            act = torch.empty(m, dtype=torch.int32, device=device)
            _lib.check(lib.cp_online_realign_activity(windows.data_ptr(), int(windows.stride(0)), m,
                                                      base.ctypes.data_as(C.POINTER(C.c_float)),
                                                      gain.ctypes.data_as(C.POINTER(C.c_float)), act.data_ptr(), stream),
                       "cp_online_realign_activity")
        else:
            act = torch.from_numpy(activity.astype(np.int32)).to(device)
        cue_d = torch.from_numpy(cue32).to(device)
        seg_d = torch.from_numpy(np.ascontiguousarray(segments, dtype=np.int32)).to(device)
        out = torch.empty(4 * n + 8 * n + m, dtype=torch.int32, device=device)    # sums (as int64) | table | expected
        c = _lib.cp_online_realign_config(*[cfg[k] for k in _PARAMS])
        _lib.check(lib.cp_online_realign(act.data_ptr(), cue_d.data_ptr(), m, seg_d.data_ptr(), n, C.byref(c),
                                         out[12 * n:].data_ptr(), out[4 * n:].data_ptr(), out.data_ptr(), stream),
                   "cp_online_realign")
        host = out.cpu().numpy()
    return host[12 * n:], host[4 * n:12 * n].reshape(n, 8), host[:4 * n].view(np.int64).reshape(n, 2)


def realign_cues(windows, cue, profile=None, *, activity=None, max_lag: int = 100, max_lead: int = 50, min_len: int = 25,
                 min_rest: int = 10, context: int = 100, min_contrast: int = 0, guard: int = 5) -> dict:
    """Move the labels of a cued recording from the cue onto the movement, on the device.  windows (M, 12) f32 on the GPU, from
    `recording_windows` or a push's `return_windows`; cue (M,) as `expected_commands` gives it (class id, REST, IGNORE).
    profile: dict(base, gain) as `activity_profile` returns it; None: `activity_profile(windows, cue)`, which fetches the
    windows to the host first.  activity=: a caller's own (M,) integer activity (clamped to 0..MAX_ACTIVITY) instead of the
    windows, for instance one made from logits; `windows` may then be None.  The settings are those of the definition
    (`realign_reference`, which the result equals in every integer), in windows: the onset lies in
    [start, start + max_lag], the offset in [end - max_lead, end + max_lag], a movement lasts min_len windows at least and
    leaves min_rest of its region (from `context` windows in front of the cue to max_lag behind it), min_contrast is the
    least difference of the two mean activities, and `guard` windows on either side of onset and offset are IGNORE.
    Returns a dict of
      expected   (M,) int64 on the host: class id, REST or IGNORE per window, for `sweep_gate`, `search_grasp_sets`,
                 `drive_profile` and `thresholds_from_logits`, and through `sample_labels` for `enroll` and `finetune`;
      segments   dict of (n_seg,) int64 columns start, end, onset, offset, status, cls, lag = onset - start and
                 overrun = offset - end (onset and offset -1, lag and overrun 0 unless status is 0 or 2);
      contrast   (n_seg,) float64 S_A / n_A - S_R / n_R of the reported pair, NaN without one.
    Every refusal is a ValueError before anything is enqueued; with a profile there is one host synchronisation, the copy
    of the results."""
    cfg = _check_params(dict(max_lag=max_lag, max_lead=max_lead, min_len=min_len, min_rest=min_rest, context=context,
                             min_contrast=min_contrast, guard=guard))
    cu = _cue_array(cue)
    m = int(cu.shape[0])
    if m < 1:
        raise ValueError("cue must hold one entry per window, and one window at least")
    device = None
    if activity is None:
        if not hasattr(windows, "data_ptr") or windows.dim() != 2 or windows.shape[1] != EMG_DIM or str(windows.dtype) != "torch.float32":
            raise ValueError(f"windows must be an (M, {EMG_DIM}) float32 tensor")
        if windows.shape[0] != m:
            raise ValueError(f"windows and cue must hold one entry per window each, got {windows.shape[0]} and {m}")
        if windows.device.type != "cuda":
            raise ValueError("windows must be on the GPU")
        device = windows.device
        if windows.stride(1) != 1 or windows.stride(0) < EMG_DIM:
            windows = windows.contiguous()
        base, gain = _check_profile(activity_profile(windows, cu) if profile is None else profile)
        act = None
    else:
        act = _activity_array(activity, m)
        if hasattr(activity, "data_ptr") and activity.device.type == "cuda":
            device = activity.device
        elif hasattr(windows, "data_ptr") and windows.device.type == "cuda":
            device = windows.device
        base = gain = None
    segs = cue_segments(cu)
    n = int(segs.shape[0])
    if n > MAX_SEGMENTS:
        raise ValueError(f"the cue has {n} segments, more than {MAX_SEGMENTS}")
    if n == 0:                                                           # nothing to move: the definition's answer, no launch
        expected, table, sums = np.where(cu < 0, cu, IGNORE), np.zeros((0, 8), dtype=np.int32), np.zeros((0, 2), dtype=np.int64)
    else:
        expected, table, sums = _realign_dev(windows, act, cu.astype(np.int32), segs, cfg, base, gain, device)
    t = table.astype(np.int64)
    has = (t[:, 6] == FOUND) | (t[:, 6] == NO_CONTRAST)
    nA = np.where(has, t[:, 5] - t[:, 4], 1)
    nR = np.where(has, t[:, 3] - t[:, 2] - nA, 1)
    contrast = np.where(has, sums[:, 0] / nA - sums[:, 1] / nR, np.nan)
    cols = dict(start=t[:, 0], end=t[:, 1], onset=t[:, 4], offset=t[:, 5], status=t[:, 6], cls=t[:, 7],
                lag=np.where(has, t[:, 4] - t[:, 0], 0), overrun=np.where(has, t[:, 5] - t[:, 1], 0))
    assert tuple(cols) == SEGMENT_COLUMNS
    return dict(expected=np.asarray(expected).astype(np.int64), segments=cols, contrast=contrast)


def sample_labels(expected, n_samples: int, phase: int = 0, rest=None) -> np.ndarray:
    """Per-sample labels for `enroll`, `finetune` and `score_channel_maps` from per-window ones: (n_samples,) int64 in which the
    samples phase + 20 k .. phase + 20 k + 19 take window k's value, REST as `rest` (None: -1, not labelled), IGNORE as -1, and
    everything outside a window's block is -1.  expected (K,) must hold the K = windows_before(n_samples, phase) windows of the
    recording.  With a `rest`, `window_labels(sample_labels(x, n, phase, rest), phase)` is x with REST -> rest and IGNORE -> -1,
    and `expected_commands` of it gives x back.  Host only (numpy)."""
    x = _cue_array(expected)
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 0:
        raise ValueError("n_samples must be a non-negative integer")
    if isinstance(phase, bool) or not isinstance(phase, (int, np.integer)) or not 0 <= phase < STRIDE:
        raise ValueError(f"phase must lie in 0..{STRIDE - 1}")
    if rest is not None and (isinstance(rest, bool) or not isinstance(rest, (int, np.integer)) or rest < 0):
        raise ValueError("rest must be None or a non-negative label")
    n, phase = int(n_samples), int(phase)
    k = max(0, (n - phase - 11 + STRIDE) // STRIDE)                      # online.windows_before
    if x.shape[0] != k:
        raise ValueError(f"expected must hold the {k} windows of {n} samples at phase {phase}, got {x.shape[0]}")
    if ((x < 0) & (x != REST) & (x != IGNORE)).any():
        raise ValueError("expected must hold class ids, REST or IGNORE")
    per_window = np.where(x >= 0, x, -1)
    if rest is not None:
        per_window = np.where(x == REST, int(rest), per_window)
    out = np.full(n, -1, dtype=np.int64)
    body = np.repeat(per_window, STRIDE)[:max(n - phase, 0)]
    out[phase:phase + body.shape[0]] = body
    return out
