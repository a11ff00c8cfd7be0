"""Prototype tracking: class rows that follow the user between enrolments.

The class rows of an online decoder are frozen from the moment `enroll` or `finetune` installs them, while over a day of wear
the user's embeddings drift (sweat, fatigue, a sleeve that creeps) and AdaBN removes only the per-channel shift and scale of
that drift.  `PrototypeTracker` is self-training on the device, a stage behind any of the four decoders as `CommandGate` is
(cp_online_track_*, csrc/online_track.cuh): windows the decoder is sure about pull their own class row along, bounded so that
a row never leaves the neighbourhood of what the user enrolled.  It reads the embeddings z / |z| that a push gives out with
`return_embeddings=True`.  `track_reference` is the definition, in numpy scalars; the device equals it in every integer and
bit.

Per stream: K class ids, ascending; anchor (K, 16) f32, the decoder's unit rows at the moment the tracker installed them;
row (K, 16) f32, the current rows, which start as the anchor; acc (K, 16) f64, the tracked direction, which starts as
float64(anchor); n_updates, n_refused (K,) integers; a ring of the last `vote` slots.

Per window with embedding e (16 f32), in window order, every operation rounded on its own (no fused multiply-add):

logits.  l[k] = sum_d e[d] * row[k][d] in f32, d ascending, from 0: the operations of the decoders' tail.
row.  k1 = 0, then every k in ascending order with l[k] > l[k1] becomes k1 (the tail's first maximum); c1 = l[k1], c2 the
maximum of the other logits (-1 for K = 1), margin = c1 - c2 in f32.
outputs.  pred = ids[k1]; k1 enters the ring, the oldest entry leaves once `vote` are in, voted = ids[the slot with the most
entries, the smallest among equals].
eligible.  rate > 0, every logit finite, c1 >= min_cosine, margin >= min_margin, and with `agree` k1 is this window's voted slot.
update, for an eligible window, in f64: a' = (1 - rate) * acc[k1] + rate * float64(e) (two products, one sum per component);
n2 = sum_d a'[d]^2, d ascending; cand = float32(a' / sqrt(n2)); in f32 ca = sum_d cand[d] * anchor[k1][d], d ascending.  If
n2 is finite and > 0 and ca >= min_anchor_cosine: acc[k1] = a', row[k1] = cand, n_updates[k1] += 1 and updated = ids[k1].
Otherwise only n_refused[k1] += 1.  updated = -1 for a refused window and for one that was not eligible.  The next window is
the first to see the new row.

So a stream's outputs do not depend on how it is cut into pushes; with rate = 0 pred, voted and logits are the decoder's own;
with min_anchor_cosine above every cosine no row ever moves.

Scores (`expected=`, as `online.expected_commands` gives it; IGNORE rows are skipped), all integers, `TRACK_SCORE_KEYS`:
n_cue (rows with a class cue), pred_hit, voted_hit (of those, pred / voted == cue), updates, refused (scored rows that
updated / were refused), wrong_updates (scored rows that updated a class other than the cue's; under REST every update),
pred_hit_tail, voted_hit_tail (the hits among the last quarter of the cue rows: those with at least n_cue - n_cue // 4 cue
rows in front of them).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib

REST, IGNORE = -1, -2                   # online.REST, online.IGNORE
D_E = _lib.CP_D_E
MAX_CLASSES = _lib.CP_ONLINE_MAX_CLASSES
MAX_VOTE = _lib.CP_ONLINE_MAX_VOTE
VOTE = 25                               # online.VOTE
MAX_CONFIGS = _lib.CP_ONLINE_TRACK_SWEEP_MAX_CONFIGS
TRACK_SCORE_KEYS = ("n_cue", "pred_hit", "voted_hit", "updates", "refused", "wrong_updates", "pred_hit_tail", "voted_hit_tail")
TRACK_KEYS = ("rate", "min_cosine", "min_margin", "min_anchor_cosine", "agree", "vote")
DEFAULTS = dict(rate=0.01, min_cosine=0.5, min_margin=0.05, min_anchor_cosine=0.7, agree=True, vote=VOTE)
_OL_STATE_BYTES, _OL_TABLE_AT = 7672, 3576          # OlState and its `table` (csrc/online.cuh; asserted in online_api.cuh)
_OT_WORDS = (16 + 4 * (MAX_CLASSES + MAX_VOTE) + 16 * MAX_CLASSES + 16 * MAX_CLASSES * D_E) // 4   # OtState in 32-bit words


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _settings(new: dict) -> dict:
    """rate, min_cosine, min_margin, min_anchor_cosine, agree, vote as the C config takes them, or ValueError"""
    extra = set(new) - set(TRACK_KEYS)
    if extra:
        raise ValueError(f"a tracker config takes {', '.join(TRACK_KEYS)}, not {sorted(extra, key=str)[0]!r}")
    s = dict(DEFAULTS)
    s.update(new)
    rate = float(s["rate"])
    if not 0.0 <= rate < 1.0:
        raise ValueError("rate must lie in [0, 1)")
    vote = s["vote"]
    if isinstance(vote, bool) or not isinstance(vote, (int, np.integer)) or not 1 <= int(vote) <= MAX_VOTE:
        raise ValueError(f"vote must lie in 1..{MAX_VOTE}")
    out = dict(rate=rate, vote=int(vote), agree=bool(s["agree"]))
    for k in ("min_cosine", "min_margin", "min_anchor_cosine"):
        v = float(np.float32(s[k]))
        if np.isnan(v):
            raise ValueError(f"{k} must not be NaN")
        out[k] = v
    return out


def _ids_array(ids) -> np.ndarray:
    cid = _host(ids).reshape(-1)
    if cid.dtype.kind not in "iu" or not 1 <= cid.shape[0] <= MAX_CLASSES:
        raise ValueError(f"ids must hold 1..{MAX_CLASSES} integer class ids")
    cid = cid.astype(np.int64)
    if (np.diff(cid) <= 0).any() or cid[0] < 0 or cid[-1] >= 2 ** 31 - 1:
        raise ValueError("ids must be ascending, distinct and in 0..2**31-2")
    return cid


def _expected_slots(expected, m: int, cid: np.ndarray) -> np.ndarray:
    """expected (M,) class ids, REST or IGNORE -> (M,) int32 class slots (REST and IGNORE as they are)"""
    exp = _host(expected)
    if exp.shape != (m,) or exp.dtype.kind not in "iu":
        raise ValueError(f"expected must hold one integer entry per window ({m})")
    exp = exp.astype(np.int64)
    pos = np.minimum(np.searchsorted(cid, exp), cid.shape[0] - 1)
    if ((exp >= 0) & (cid[pos] != exp)).any() or (exp < IGNORE).any():
        raise ValueError("expected holds class ids among ids, REST or IGNORE")
    return np.where(exp >= 0, pos, exp).astype(np.int32)


def _tail_from(slots: np.ndarray) -> int:
    n_cue = int((slots >= 0).sum())
    return n_cue - n_cue // 4


def fresh_state(rows, ids) -> dict:
    """The state `track_reference` starts from: rows (K, 16) f32 unit rows taken as they are, ids (K,) ascending."""
    cid = _ids_array(ids)
    anchor = np.array(_host(rows), dtype=np.float32).reshape(-1, D_E)
    if anchor.shape[0] != cid.shape[0]:
        raise ValueError("one row of 16 per id")
    k = cid.shape[0]
    return dict(ids=cid, anchor=anchor.copy(), rows=anchor.copy(), acc=anchor.astype(np.float64),
                n_updates=np.zeros(k, dtype=np.int64), n_refused=np.zeros(k, dtype=np.int64), ring=[])


def track_reference(embeddings, rows=None, ids=None, *, state: Optional[dict] = None, expected=None, **settings) -> dict:
    """The definition of the tracker (module docstring), in numpy scalars: embeddings (M, 16) f32 through a tracker that starts
    fresh on rows (K, 16), ids (K,), or continues from `state` (the "state" entry of an earlier call; it is not modified).
    settings: rate, min_cosine, min_margin, min_anchor_cosine, agree, vote (`DEFAULTS`).  Returns a dict: pred, voted, updated
    (M,) int64 class ids (updated -1: none), logits (M, K) f32, state (ids, anchor, rows (K, 16) f32, acc (K, 16) f64, n_updates,
    n_refused (K,) int64, ring: the slots in it from the oldest to the newest), and with expected= scores, a dict with
    `TRACK_SCORE_KEYS`.  Host only."""
    s = _settings(settings)
    st = fresh_state(rows, ids) if state is None else state
    cid = np.asarray(st["ids"], dtype=np.int64)
    k = cid.shape[0]
    anchor = np.array(st["anchor"], dtype=np.float32)
    row = np.array(st["rows"], dtype=np.float32)
    acc = np.array(st["acc"], dtype=np.float64)
    n_up, n_ref = np.array(st["n_updates"], dtype=np.int64), np.array(st["n_refused"], dtype=np.int64)
    vote = s["vote"]
    ring = list(st["ring"])[-vote:]
    cnt = np.bincount(np.asarray(ring, dtype=np.int64), minlength=k) if ring else np.zeros(k, dtype=np.int64)
    emb = np.array(_host(embeddings), dtype=np.float32).reshape(-1, D_E)
    m = emb.shape[0]
    beta, keep = np.float64(s["rate"]), np.float64(1.0) - np.float64(s["rate"])
    min_cos, min_mar, min_anc = np.float32(s["min_cosine"]), np.float32(s["min_margin"]), np.float32(s["min_anchor_cosine"])
    pred, voted, updated = (np.zeros(m, dtype=np.int64) for _ in range(3))
    slots = np.zeros((m, 3), dtype=np.int64)
    refused = np.zeros(m, dtype=bool)
    logits = np.zeros((m, k), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(m):
            e = emb[j]
            l = np.zeros(k, dtype=np.float32)
            for d in range(D_E):
                l = l + e[d] * row[:, d]                   # (two f32 array operations: every product and sum is rounded)
            logits[j] = l
            k1 = 0
            for c in range(1, k):
                if l[c] > l[k1]:
                    k1 = c
            c1 = l[k1]
            c2 = np.float32(-1.0) if k == 1 else np.max(np.delete(l, k1))
            margin = np.float32(c1 - c2)
            if len(ring) == vote:
                cnt[ring.pop(0)] -= 1
            ring.append(k1)
            cnt[k1] += 1
            vj = int(np.argmax(cnt))                       # the first maximum: the smallest slot among equals
            pred[j], voted[j], updated[j] = cid[k1], cid[vj], -1
            slots[j] = k1, vj, -1
            if not (beta > 0 and np.isfinite(l).all() and c1 >= min_cos and margin >= min_mar and (not s["agree"] or k1 == vj)):
                continue
            a2 = keep * acc[k1] + beta * e.astype(np.float64)
            n2 = np.float64(0.0)
            for d in range(D_E):
                n2 = n2 + a2[d] * a2[d]
            cand = (a2 / np.sqrt(n2)).astype(np.float32)
            ca = np.float32(0.0)
            for d in range(D_E):
                ca = ca + cand[d] * anchor[k1, d]
            if np.isfinite(n2) and n2 > 0 and ca >= min_anc:
                acc[k1], row[k1] = a2, cand
                n_up[k1] += 1
                updated[j] = cid[k1]
                slots[j, 2] = k1
            else:
                n_ref[k1] += 1
                refused[j] = True
    out = dict(pred=pred, voted=voted, updated=updated, logits=logits,
               state=dict(ids=cid, anchor=anchor, rows=row, acc=acc, n_updates=n_up, n_refused=n_ref, ring=ring))
    if expected is not None:
        ex = _expected_slots(expected, m, cid).astype(np.int64)
        cue, scored = ex >= 0, ex >= REST
        tail = cue & (np.cumsum(cue) - 1 >= _tail_from(ex))
        upd = scored & (slots[:, 2] >= 0)
        sc = (cue.sum(), (cue & (slots[:, 0] == ex)).sum(), (cue & (slots[:, 1] == ex)).sum(), upd.sum(), (scored & refused).sum(),
              (upd & (slots[:, 2] != ex)).sum(), (tail & (slots[:, 0] == ex)).sum(), (tail & (slots[:, 1] == ex)).sum())
        out["scores"] = {key: int(v) for key, v in zip(TRACK_SCORE_KEYS, sc)}
    return out


def drifting_stream(n_rows: int, k: int, seed: int = 0, noise: float = 0.25, degrees: float = 40.0, segment: int = 50, rest_every: int = 0):
    """A synthetic cued recording whose embeddings drift, for tests and measurements; nothing about real subjects.  Returns
    (embeddings (n_rows, 16) f32 unit rows, expected (n_rows,) int64 slots 0..k-1 or REST, rows (k, 16) f32 unit class rows).
    The cue walks through the classes in segments of `segment` rows (every `rest_every`-th segment is REST, 0: none, and a
    REST row is noise alone); a cued row is its class row plus `noise` * a standard normal vector, turned in each of the eight
    coordinate planes (0, 1), (2, 3), .. (14, 15) by a Givens rotation whose angle grows linearly from 0 to `degrees` over the
    recording, and normalised.  Host only; the same arrays for the same arguments."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((k, D_E))
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    emb = np.zeros((n_rows, D_E), dtype=np.float64)
    exp = np.zeros(n_rows, dtype=np.int64)
    order = rng.permutation(k)
    for j in range(n_rows):
        seg = j // segment
        rest = rest_every > 0 and seg % rest_every == rest_every - 1
        c = int(order[seg % k])
        v = noise * rng.standard_normal(D_E)
        if not rest:
            v = v + rows[c].astype(np.float64)
        t = np.deg2rad(degrees) * j / max(n_rows - 1, 1)
        for a in range(0, D_E, 2):
            b = a + 1
            va, vb = v[a], v[b]
            v[a], v[b] = np.cos(t) * va - np.sin(t) * vb, np.sin(t) * va + np.cos(t) * vb
        emb[j] = v / np.linalg.norm(v)
        exp[j] = REST if rest else c
    return emb.astype(np.float32), exp, rows


def pick_tracker(scores, max_wrong_rate: float = 0.02):
    """The index of the setting to use, from the scores of `sweep_tracker` (a dict of (G,) arrays): among the settings with
    wrong_updates / updates <= max_wrong_rate (no updates: rate 0) the one with the most voted hits in the last quarter of
    the cue rows, then the most voted hits, then the smallest index; None if no setting is eligible."""
    sc = {k: np.asarray(scores[k], dtype=np.int64).reshape(-1) for k in TRACK_SCORE_KEYS}
    rate = np.where(sc["updates"] > 0, sc["wrong_updates"] / np.maximum(sc["updates"], 1), 0.0)
    idx = np.nonzero((rate <= max_wrong_rate) & (sc["n_cue"] >= 0))[0]
    if idx.size == 0:
        return None
    return int(min(idx.tolist(), key=lambda g: (-int(sc["voted_hit_tail"][g]), -int(sc["voted_hit"][g]), g)))


def track_grid(**lists) -> list:
    """The cartesian product of lists of tracker settings as a list of config dicts, the last name varying fastest."""
    import itertools
    extra = set(lists) - set(TRACK_KEYS)
    if extra:
        raise ValueError(f"a tracker config takes {', '.join(TRACK_KEYS)}, not {sorted(extra)[0]!r}")
    names = list(lists)
    return [dict(zip(names, combo)) for combo in itertools.product(*(list(lists[n]) for n in names))]


def _config_struct(s: dict):
    c = _lib.cp_online_track_config()
    c.vote, c.agree, c.rate = s["vote"], int(s["agree"]), s["rate"]
    c.min_cosine, c.min_margin, c.min_anchor_cosine = s["min_cosine"], s["min_margin"], s["min_anchor_cosine"]
    return c


_CONFIG_DTYPE = np.dtype([("vote", "<i4"), ("agree", "<i4"), ("rate", "<f8"), ("min_cosine", "<f4"), ("min_margin", "<f4"),
                          ("min_anchor_cosine", "<f4"), ("reserved0", "<i4")])
assert _CONFIG_DTYPE.itemsize == C.sizeof(_lib.cp_online_track_config)


def sweep_tracker(embeddings, expected, ids, rows, configs, return_sequences: bool = False):
    """Score many tracker settings over one cued recording's embeddings in one pass on the device (cp_online_track_sweep: one
    wave per setting, each from a fresh tracker on `rows`).  embeddings (M, 16) f32 on the GPU (`embed_recording`); expected
    (M,) as `online.expected_commands` gives it; ids the K ascending class ids; rows (K, 16) f32 unit rows (what
    `PrototypeTracker.rows` or `track_reference` hold as the anchor); configs a sequence of dicts with `TRACK_KEYS`, missing
    keys at `DEFAULTS`, checked before anything is enqueued.  Returns {key: (G,) int64 array} with `TRACK_SCORE_KEYS`: setting
    g's entry is the `scores` of `track_reference` with that setting.  return_sequences=True: (scores, pred, voted, updated),
    each (G, M) int32 class ids on the GPU (updated -1: none), the sequences a fresh `PrototypeTracker` returns.  One host
    synchronisation: the copy of the score table."""
    import torch
    cid = _ids_array(ids)
    configs = list(configs)
    if not 1 <= len(configs) <= MAX_CONFIGS:
        raise ValueError(f"sweep_tracker takes 1..{MAX_CONFIGS} configs, got {len(configs)}")
    cfg = np.zeros(len(configs), dtype=_CONFIG_DTYPE)
    for g, c in enumerate(configs):
        if not isinstance(c, dict):
            raise ValueError(f"config {g} is not a dict")
        s = _settings(c)
        cfg[g] = (s["vote"], int(s["agree"]), s["rate"], s["min_cosine"], s["min_margin"], s["min_anchor_cosine"], 0)
    if not isinstance(embeddings, torch.Tensor) or embeddings.dtype != torch.float32 or embeddings.dim() != 2 \
            or embeddings.shape[1] != D_E:
        raise ValueError("embeddings must be an (M, 16) float32 tensor")
    m, g, k = int(embeddings.shape[0]), len(configs), int(cid.shape[0])
    slots = _expected_slots(expected, m, cid)
    dev = embeddings.device
    if m and dev.type != "cuda":
        raise ValueError("embeddings must be on the GPU")
    rows_t = torch.as_tensor(_host(rows), dtype=torch.float32).reshape(-1, D_E)
    if rows_t.shape[0] != k:
        raise ValueError("one row of 16 per id")
    if m == 0:
        scores = np.zeros((g, len(TRACK_SCORE_KEYS)), dtype=np.int64)
        seq = [torch.empty(g, 0, dtype=torch.int32, device=dev) for _ in range(3)]
    else:
        lib = _lib.load()
        with torch.cuda.device(dev):
            emb = embeddings.contiguous()
            if emb.data_ptr() % 16:
                emb = emb.clone()
            rows_d = rows_t.to(dev).contiguous()
            exp_d = torch.from_numpy(slots).to(dev)
            cfg_d = torch.from_numpy(cfg.view(np.uint8).reshape(g, -1)).to(dev)
            sc_d = torch.empty(g, len(TRACK_SCORE_KEYS), dtype=torch.int64, device=dev)
            seq = [torch.empty(g, m, dtype=torch.int32, device=dev) for _ in range(3)] if return_sequences else [None] * 3
            _lib.check(lib.cp_online_track_sweep(emb.data_ptr(), m, k, rows_d.data_ptr(), exp_d.data_ptr(), _tail_from(slots),
                                                 cfg_d.data_ptr(), g, sc_d.data_ptr(), *(None if t is None else t.data_ptr() for t in seq),
                                                 torch.cuda.current_stream(dev).cuda_stream), "cp_online_track_sweep")
            scores = sc_d.cpu().numpy()
            if return_sequences:                           # slots -> class ids
                table = torch.from_numpy(np.concatenate([[-1], cid]).astype(np.int32)).to(dev)
                seq = [table[(t + 1).long()] for t in seq]
    out = {key: scores[:, i].copy() for i, key in enumerate(TRACK_SCORE_KEYS)}
    return (out, *seq) if return_sequences else out


def embed_recording(decoder, raw, stream: Optional[int] = None):
    """The embeddings (M, 16) f32 of a cued recording raw (n, 12) f32 on the GPU, as a fresh stream of `decoder` emits them:
    the stream (of a multi-stream decoder: `stream`) is reset, the recording is pushed in chunks with return_embeddings=True,
    and the stream is reset again.  The adaptive forms track the recording with their alpha as any push does."""
    import torch
    multi = isinstance(decoder.class_ids, (list, tuple))
    if multi and stream is None:
        raise ValueError("embed_recording(decoder, raw, stream) on a multi-stream decoder")
    step = _lib.CP_ONLINE_STRIDE * decoder.max_windows
    parts = []
    if multi:
        decoder.reset([stream])
        for lo in range(0, raw.shape[0], step):
            chunks = [None] * decoder.n_streams
            chunks[stream] = raw[lo:lo + step]
            parts.append(decoder.push(chunks, return_embeddings=True)[stream][-1])
        decoder.reset([stream])
    else:
        decoder.reset()
        for lo in range(0, raw.shape[0], step):
            parts.append(decoder.push(raw[lo:lo + step], return_embeddings=True)[-1])
        decoder.reset()
    if not parts:
        return torch.empty(0, D_E, dtype=torch.float32, device=decoder.device)
    return parts[0] if len(parts) == 1 else torch.cat(parts)


class PrototypeTracker:
    """Class rows that follow the user, behind any of the four decoders: per stream one state machine on the device that
    reads the embeddings of every push (include/cpnative.h, cp_online_track_*; one launch more per push, nothing is copied
    to the host).  The module docstring has the definition.

    rate: beta in [0, 1), the share of an accepted window in its class's tracked direction (0: nothing moves, and pred, voted
    and logits are the decoder's own bit for bit); min_cosine, min_margin: the top cosine and its lead over the runner-up that
    an updating window must reach; min_anchor_cosine: a row never falls below this cosine to its enrolled row; agree: only a
    window whose class is also the voted class updates; vote: the ring length (default: the decoder's).

    The tracker's outputs replace the decoder's: its `pred` and `voted` come from the tracked rows, its logits feed
    `CommandGate.apply` and its class ids `GraspDrive.apply`.  The decoder's own rows stay as they are until `adopt` writes the
    tracked rows into it.  The tracker follows the decoder: a new `class_ids` object (set_classes, enroll, finetune, refresh,
    adopt) makes it take the decoder's unit rows as its new anchor before the next launch, and a push or reset of the decoder
    behind its back makes the next `push` raise `CpNativeError` before anything is enqueued."""

    def __init__(self, decoder, rate: float = DEFAULTS["rate"], min_cosine: float = DEFAULTS["min_cosine"],
                 min_margin: float = DEFAULTS["min_margin"], min_anchor_cosine: float = DEFAULTS["min_anchor_cosine"],
                 agree: bool = DEFAULTS["agree"], vote: Optional[int] = None):
        for name in ("class_ids", "n_seen", "vote", "push", "ws"):
            if not hasattr(decoder, name):
                raise TypeError("PrototypeTracker wraps an OnlineDecoder, MultiStreamDecoder or AdaptiveMultiStreamDecoder")
        self.decoder = decoder
        self.multi = isinstance(decoder.class_ids, (list, tuple))
        self.n_streams = len(decoder.class_ids) if self.multi else 1
        self.settings = _settings(dict(rate=rate, min_cosine=min_cosine, min_margin=min_margin, min_anchor_cosine=min_anchor_cosine,
                                       agree=agree, vote=decoder.vote if vote is None else vote))
        self.vote = self.settings["vote"]
        self._cfg = _config_struct(self.settings)
        self._ids_seen = [None] * self.n_streams            # the class_ids object each stream's anchor was installed from
        self._ids = [None] * self.n_streams                 # its ids (K,) int64
        self.device = decoder.device
        self.ws = None                                      # allocated with the first launch
        self._rows_cache = {}
        self._left = self._seen_now()

    # ------------------------------------------------------------------ settings
    def set(self, **kw):
        """Change rate, min_cosine, min_margin, min_anchor_cosine or agree from the next window on (vote is fixed at
        construction: the ring is laid out by it)."""
        if "vote" in kw:
            raise ValueError("vote is fixed at construction: the ring is laid out by it")
        new = dict(self.settings)
        new.update(kw)
        self.settings = _settings(new)
        self._cfg = _config_struct(self.settings)

    def use(self, config: dict):
        """Apply one config of `sweep_tracker` / `track_grid`; a config that names another vote is refused."""
        if "vote" in config and config["vote"] != self.vote:
            raise ValueError("vote is fixed at construction: the ring is laid out by it")
        self.set(**{k: v for k, v in config.items() if k != "vote"})

    # ------------------------------------------------------------------ the device side (one method per C entry)
    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _args(self):
        if self.ws is None:
            import torch
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_track_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return C.byref(self._cfg), self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_set_rows(self, s: int, ids: np.ndarray, rows):
        k = int(ids.shape[0])
        args = self._args()
        _lib.check(self.lib.cp_online_track_set_rows(*args, s, (C.c_int32 * k)(*ids.tolist()), rows.data_ptr(), k, self._stream()),
                   "cp_online_track_set_rows")

    def _dev_reset(self, s: int, rows: bool):
        args = self._args()
        what = _lib.CP_ONLINE_TRACK_RESET_ROWS if rows else _lib.CP_ONLINE_TRACK_RESET_RING
        _lib.check(self.lib.cp_online_track_reset(*args, s, what, self._stream()), "cp_online_track_reset")

    def _dev_push(self, emb, row0: np.ndarray, m: np.ndarray, rows: int, want_logits: bool):
        """one launch over `rows` packed rows -> (pred, voted, updated) (3, rows) int32 and logits (rows, 64) f32 or None"""
        import torch
        from .online import _rows_on_device
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.device)
        pvu = torch.empty(3, rows, dtype=torch.int32, device=self.device)
        logits = torch.empty(rows, MAX_CLASSES, dtype=torch.float32, device=self.device) if want_logits else None
        _lib.check(self.lib.cp_online_track_push(*args, emb.data_ptr(), rm[0].data_ptr(), rm[1].data_ptr(), rows, pvu[0].data_ptr(),
                                                 pvu[1].data_ptr(), logits.data_ptr() if want_logits else None, MAX_CLASSES,
                                                 pvu[2].data_ptr(), self._stream()), "cp_online_track_push")
        return pvu, logits

    # ------------------------------------------------------------------ staying in step with the decoder
    def _seen_now(self) -> np.ndarray:
        return np.array(self.decoder.n_seen, dtype=np.int64).reshape(-1).copy()

    def _class_ids(self, s: int):
        return self.decoder.class_ids[s] if self.multi else self.decoder.class_ids

    def _unit_rows(self, s: int, k: int):
        """the decoder's normalised class table of stream s, (k, 16) f32, bit for bit as its tail reads it: the decoders keep
        one OlState per stream at the start of their workspace, the table behind the ids (csrc/online.cuh)"""
        import torch
        at = s * _OL_STATE_BYTES + _OL_TABLE_AT
        return self.decoder.ws[at:at + k * D_E * 4].view(torch.float32).reshape(k, D_E).clone()

    def _sync_classes(self):
        for s in range(self.n_streams):
            cur = self._class_ids(s)
            if cur is None or cur is self._ids_seen[s]:
                continue
            ids = _ids_array(cur)
            self._dev_set_rows(s, ids, self._unit_rows(s, int(ids.shape[0])))
            self._ids_seen[s] = cur
            self._ids[s] = ids

    def _check_in_step(self):
        if not np.array_equal(self._seen_now(), self._left):
            raise _lib.CpNativeError("the decoder was pushed or reset behind the tracker (its n_seen is not what the tracker left): "
                                     "the tracker's ring no longer follows the stream; push and reset through the tracker, or "
                                     "reset() it")

    # ------------------------------------------------------------------ the stage over per-stream embeddings
    def _track(self, per_stream, want_logits: bool):
        """per_stream: n_streams entries, None or (M_s, 16) f32 embeddings -> per stream (pred, voted, logits or None, updated)"""
        import torch
        self._sync_classes()
        step = _lib.CP_ONLINE_MAX_WINDOWS
        ms = []
        for s, t in enumerate(per_stream):
            if t is None:
                ms.append(0)
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != D_E \
                    or t.device.type != "cuda":
                raise ValueError("embeddings must be (M, 16) float32 tensors on the GPU")
            if t.shape[0] and self._ids_seen[s] is None:
                raise _lib.CpNativeError(f"stream {s} has embeddings but no class list: set_classes on the decoder first")
            ms.append(int(t.shape[0]))
        outs = []
        for lo in range(0, max(max(ms), 1), step):
            m = np.array([min(max(n - lo, 0), step) for n in ms], dtype=np.int64)
            rows = int(m.sum())
            row0 = np.zeros_like(m)
            np.cumsum(m[:-1], out=row0[1:])
            if rows == 0:
                pvu = torch.empty(3, 0, dtype=torch.int32, device=self.device)
                logits = torch.empty(0, MAX_CLASSES, dtype=torch.float32, device=self.device) if want_logits else None
            else:
                views = [per_stream[s][lo:lo + n] for s, n in enumerate(m.tolist()) if n]
                base = views[0]
                packed = base.stride() == (D_E, 1) and base.data_ptr() % 16 == 0
                for v, r in zip(views, row0[m > 0].tolist()):   # the packed output of one push lies as the launch reads it
                    packed = packed and v.stride() == (D_E, 1) and v.data_ptr() == base.data_ptr() + 4 * D_E * r
                emb = base if packed else torch.cat(views).contiguous()
                pvu, logits = self._dev_push(emb, row0, m, rows, want_logits)
            ml = m.tolist()
            lg = [None] * self.n_streams if logits is None else \
                [x[:, :(0 if i is None else i.shape[0])] for x, i in zip(logits.split(ml), self._ids)]
            outs.append(list(zip(pvu[0].split(ml), pvu[1].split(ml), lg, pvu[2].split(ml))))
        if len(outs) == 1:
            return outs[0]
        return [tuple(None if outs[0][s][i] is None else torch.cat([o[s][i] for o in outs]) for i in range(4))
                for s in range(self.n_streams)]

    # ------------------------------------------------------------------ API
    def apply(self, embeddings, return_logits: bool = False):
        """The stage alone on embeddings the caller already has (of the decoder's next windows, in order): (M, 16) f32 on the
        GPU -> (pred, voted[, logits], updated); on a multi-stream decoder a list with one entry per stream (None: no windows)
        -> one such tuple per stream.  pred, voted (M,) int32 class ids, logits (M, K) f32, updated (M,) int32 class id or -1."""
        import torch
        if self.multi:
            if isinstance(embeddings, torch.Tensor) or len(embeddings) != self.n_streams:
                raise ValueError(f"embeddings must be a sequence of {self.n_streams} entries (None or (M, 16) tensors)")
            out = [self._pick(t, return_logits) for t in self._track(list(embeddings), return_logits)]
        else:
            out = self._pick(self._track([embeddings], return_logits)[0], return_logits)
        self._left = self._seen_now()
        return out

    @staticmethod
    def _pick(t, return_logits: bool, windows=None):
        res = [t[0], t[1]]
        if return_logits:
            res.append(t[2])
        if windows is not None:
            res.append(windows)
        return tuple(res) + (t[3],)

    def push(self, raw, return_logits: bool = False, return_windows: bool = False):
        """What the decoder's `push` takes (raw (n, 12), or one chunk per stream) -> (pred, voted[, logits][, windows], updated)
        per stream, pred, voted and logits from the tracked rows."""
        self._check_in_step()
        self._sync_classes()
        res = self.decoder.push(raw, return_windows=return_windows, return_embeddings=True)
        return self._finish(res, return_logits, return_windows)

    def push_packed(self, raw, counts, return_logits: bool = False, return_windows: bool = False):
        """`push` for samples packed in stream order, as the multi-stream decoders' `push_packed`."""
        if not self.multi:
            raise TypeError("push_packed belongs to the multi-stream decoders")
        self._check_in_step()
        self._sync_classes()
        res = self.decoder.push_packed(raw, counts, return_windows=return_windows, return_embeddings=True)
        return self._finish(res, return_logits, return_windows)

    def _finish(self, res, return_logits: bool, return_windows: bool):
        self._left = self._seen_now()
        if self.multi:
            tracked = self._track([r[-1] for r in res], return_logits)
            return [self._pick(t, return_logits, r[2] if return_windows else None) for r, t in zip(res, tracked)]
        return self._pick(self._track([res[-1]], return_logits)[0], return_logits, res[2] if return_windows else None)

    def _index(self, stream) -> int:
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {stream!r}")
        return int(stream)

    def rows(self, stream: int = 0):
        """(rows (K, 16) f32 on the GPU, ids (K,) int64, n_updates (K,), n_refused (K,) int64 numpy) of one stream: the current
        rows and how often each class was updated and refused since the anchor was installed (this waits for the device)."""
        import torch
        s = self._index(stream)
        self._sync_classes()
        if self._ids[s] is None:
            raise _lib.CpNativeError(f"stream {s} has no class list: set_classes on the decoder first")
        k = int(self._ids[s].shape[0])
        args = self._args()
        rows = torch.empty(MAX_CLASSES, D_E, dtype=torch.float32, device=self.device)
        cnt = torch.empty(2, MAX_CLASSES, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.cp_online_track_rows(*args, s, rows.data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), self._stream()),
                   "cp_online_track_rows")
        c = cnt.cpu().numpy()
        return rows[:k].clone(), self._ids[s].copy(), c[0, :k].copy(), c[1, :k].copy()

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back in the layout of `track_reference`'s state (this waits for
        the device; a test and debugging aid).  The layout is that of OtState (csrc/online_track.cuh): int32 K, head, len, one
        unused, ids[64], ring[256]; int64 n_updates[64], n_refused[64]; f32 anchor[64][16], row[64][16]; f64 acc[64][16]."""
        s = self._index(stream)
        self._sync_classes()
        if self.ws is None or self._ids[s] is None:
            raise _lib.CpNativeError(f"stream {s} has no class list: set_classes on the decoder first")
        nb = _OT_WORDS * 4
        raw = self.ws[s * nb:(s + 1) * nb].cpu().numpy()
        w = raw.view(np.int32)
        k, head, n = int(w[0]), int(w[1]), int(w[2])
        at = 16 + 4 * (MAX_CLASSES + MAX_VOTE)
        cnt = raw[at:at + 16 * MAX_CLASSES].view(np.int64).reshape(2, MAX_CLASSES)
        at += 16 * MAX_CLASSES
        f = raw[at:at + 8 * MAX_CLASSES * D_E].view(np.float32).reshape(2, MAX_CLASSES, D_E)
        at += 8 * MAX_CLASSES * D_E
        acc = raw[at:at + 8 * MAX_CLASSES * D_E].view(np.float64).reshape(MAX_CLASSES, D_E)
        ring = w[4 + MAX_CLASSES:4 + MAX_CLASSES + MAX_VOTE]
        return dict(ids=w[4:4 + k].astype(np.int64), anchor=f[0, :k].copy(), rows=f[1, :k].copy(), acc=acc[:k].copy(),
                    n_updates=cnt[0, :k].copy(), n_refused=cnt[1, :k].copy(),
                    ring=[int(ring[(head - n + i) % self.vote]) for i in range(n)])

    def reset(self, streams=None, rows: bool = False):
        """Reset the decoder and the tracker's ring; rows=True also puts the tracked rows back to the anchor and the counters
        to 0.  On a multi-stream decoder the listed streams, default all."""
        self._sync_classes()
        if self.multi and streams is not None:
            idx = sorted({self._index(s) for s in streams})
            self.decoder.reset(idx)
            for s in idx:
                self._dev_reset(s, rows)
        else:
            self.decoder.reset()
            self._dev_reset(-1, rows)
        self._left = self._seen_now()

    def adopt(self, stream: int = 0):
        """Write the tracked rows of one stream into the decoder, through its `set_classes(table=..., ids=...)`: this is how a
        user keeps the rows (`class_table()` then returns them).  The decoder normalises a table it is given, so what it holds
        afterwards can differ from the tracked rows in the last bit; the tracker takes the decoder's rows as its new anchor
        (a new `class_ids` object), so that the two stay bit-identical, and its counters start again.  The vote rings empty, as
        after any `set_classes`."""
        s = self._index(stream)
        rows, ids, _, _ = self.rows(s)
        if self.multi:
            self.decoder.set_classes(s, table=rows, ids=ids)
        else:
            self.decoder.set_classes(table=rows, ids=ids)
        self._sync_classes()
