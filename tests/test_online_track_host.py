"""Prototype tracking without a GPU (contrastiveprosthetics_amd/track.py, include/cpnative.h cp_online_track_*): the properties
of the numpy definition `track_reference` on a seeded synthetic stream, what tracking buys on a drifting one, and the host
checks of every new C entry."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from contrastiveprosthetics_amd import track as T
from contrastiveprosthetics_amd.track import track_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cpnative.h")
LIB = os.path.join(ROOT, "contrastiveprosthetics_amd", "libcpnative.so")
ERR_ARG = 10001
F = np.float32
EMBED = ["cp_online_push_embed", "cp_online_adapt_push_embed", "cp_online_multi_push_embed", "cp_online_multi_adapt_push_embed"]
TRACK = ["cp_online_track_workspace_bytes", "cp_online_track_set_rows", "cp_online_track_reset", "cp_online_track_push",
         "cp_online_track_rows", "cp_online_track_sweep"]

# the drifting stream of this file and of tests/test_gpu_online_track.py: 41 classes, noise 0.4, 40 degrees; fixed here so that
# the numpy definition alone meets `test_tracking_beats_frozen_rows_on_the_drifting_stream`
DRIFT = dict(n_rows=2400, k=41, seed=3, noise=0.4, degrees=40.0, segment=50)
DRIFT_SETTINGS = dict(rate=0.05, min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.5, agree=True, vote=25)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_state(a, b):
    return all(same_bits(a[k], b[k]) for k in ("ids", "anchor", "rows", "acc", "n_updates", "n_refused")) and a["ring"] == b["ring"]


def stream(n=500, k=7, seed=1):
    emb, exp, rows = T.drifting_stream(n, k, seed=seed, noise=0.3, degrees=25.0, segment=20, rest_every=4)
    ids = np.arange(k) * 3 + 2                                         # class ids that are not their slots
    return emb, np.where(exp >= 0, ids[np.maximum(exp, 0)], exp), rows, ids


# ---------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------
def static_decode(emb, rows, ids, vote):
    """argmax (first maximum) of sequential f32 cosines and the mode of the last `vote` of them, as the decoders do it"""
    l = np.zeros((emb.shape[0], rows.shape[0]), dtype=F)
    for d in range(16):
        l = l + emb[:, d:d + 1] * rows[None, :, d]
    k1 = l.argmax(axis=1)
    voted = np.array([np.bincount(k1[max(0, j - vote + 1):j + 1], minlength=rows.shape[0]).argmax() for j in range(len(k1))])
    return l, ids[k1], ids[voted]


@pytest.mark.parametrize("vote", [1, 5, 25])
def test_rate_zero_is_the_static_argmax_and_vote(vote):
    emb, exp, rows, ids = stream()
    out = track_reference(emb, rows, ids, rate=0.0, vote=vote, min_cosine=-2.0, min_margin=0.0, min_anchor_cosine=-2.0, agree=False)
    l, pred, voted = static_decode(emb, rows, ids, vote)
    assert same_bits(out["logits"], l) and np.array_equal(out["pred"], pred) and np.array_equal(out["voted"], voted)
    assert (out["updated"] == -1).all() and out["state"]["n_updates"].sum() == 0 and out["state"]["n_refused"].sum() == 0
    assert same_bits(out["state"]["rows"], rows) and same_bits(out["state"]["acc"], rows.astype(np.float64))


@pytest.mark.parametrize("agree", [False, True])
def test_a_cut_into_pieces_carrying_the_state_equals_the_whole(agree):
    emb, exp, rows, ids = stream()
    kw = dict(rate=0.1, min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.6, agree=agree, vote=9)
    whole = track_reference(emb, rows, ids, **kw)
    assert (whole["updated"] >= 0).sum() > 50
    state, parts, p = None, [], 0
    for n in (1, 16, 17, 0, 255, 3, emb.shape[0] - 292):
        out = track_reference(emb[p:p + n], rows, ids, state=state, **kw)
        state = out["state"]
        parts.append(out)
        p += n
    assert p == emb.shape[0]
    for key in ("pred", "voted", "updated", "logits"):
        assert same_bits(np.concatenate([o[key] for o in parts]), whole[key]), key
    assert same_state(state, whole["state"])
    assert not same_bits(whole["state"]["rows"], rows)                 # rows moved


def test_an_anchor_bound_just_under_one_gives_only_refusals():
    emb, exp, rows, ids = stream()
    kw = dict(rate=0.1, min_cosine=0.3, min_margin=0.02, agree=False, vote=9)
    free = track_reference(emb, rows, ids, min_anchor_cosine=-2.0, **kw)
    held = track_reference(emb, rows, ids, min_anchor_cosine=float(np.nextafter(F(1), F(0))), **kw)
    frozen = track_reference(emb, rows, ids, **dict(kw, rate=0.0), min_anchor_cosine=-2.0)
    assert free["state"]["n_updates"].sum() > 50 and free["state"]["n_refused"].sum() == 0
    assert held["state"]["n_updates"].sum() == 0 and held["state"]["n_refused"].sum() > 50 and (held["updated"] == -1).all()
    assert same_bits(held["state"]["rows"], rows) and same_bits(held["state"]["acc"], rows.astype(np.float64))
    for key in ("pred", "voted", "logits"):                            # nothing moved: the frozen decoder's outputs
        assert same_bits(held[key], frozen[key]), key


def test_rows_that_are_not_numbers_never_update():
    emb, exp, rows, ids = stream(n=120)
    emb = emb.copy()
    emb[10, 3], emb[20, 0], emb[30] = np.nan, np.inf, 0.0
    emb[40], emb[41, 5] = np.nan, -np.inf
    out = track_reference(emb, rows, ids, rate=0.1, min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.5, agree=False, vote=5)
    assert (out["updated"][[10, 20, 30, 40, 41]] == -1).all() and (out["updated"] >= 0).sum() > 20
    assert np.isfinite(out["state"]["rows"]).all() and np.isfinite(out["state"]["acc"]).all()
    assert out["pred"][40] == ids[0]                                   # a NaN in slot 0 stays the maximum, as in the tail's loop


def test_scores_count_what_they_say():
    emb, exp, rows, ids = stream()
    out = track_reference(emb, rows, ids, expected=exp, rate=0.1, min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.5, vote=5)
    sc, cue, scored = out["scores"], exp >= 0, exp >= T.REST
    assert tuple(sc) == T.TRACK_SCORE_KEYS
    assert sc["n_cue"] == cue.sum() and sc["pred_hit"] == (cue & (out["pred"] == exp)).sum()
    assert sc["voted_hit"] == (cue & (out["voted"] == exp)).sum()
    assert sc["updates"] == (scored & (out["updated"] >= 0)).sum()
    assert sc["wrong_updates"] == (scored & (out["updated"] >= 0) & (out["updated"] != exp)).sum()
    last = np.nonzero(cue)[0][sc["n_cue"] - sc["n_cue"] // 4:]
    assert sc["voted_hit_tail"] == (out["voted"][last] == exp[last]).sum() and sc["pred_hit_tail"] == (out["pred"][last] == exp[last]).sum()
    assert 0 < sc["voted_hit_tail"] < sc["voted_hit"]


def test_tracking_beats_frozen_rows_on_the_drifting_stream():
    """a condition on the input, not a measurement: the seed, noise and rate above are chosen so that the definition itself
    scores strictly more voted hits in the last quarter with tracking on, with under 2 % of its updates under another cue"""
    emb, exp, rows = T.drifting_stream(**DRIFT)
    ids = np.arange(DRIFT["k"])
    frozen = track_reference(emb, rows, ids, expected=exp, **dict(DRIFT_SETTINGS, rate=0.0))["scores"]
    moving = track_reference(emb, rows, ids, expected=exp, **DRIFT_SETTINGS)["scores"]
    print(frozen, moving)
    angle = np.degrees(np.arccos(np.clip((emb[-50:] @ rows[exp[-50:]].T).diagonal().mean() / (emb[:50] @ rows[exp[:50]].T).diagonal().mean(), -1, 1)))
    assert 30 < angle < 50, angle                                      # the drift is there: about 40 degrees at the end
    assert frozen["updates"] == 0
    assert moving["voted_hit_tail"] > frozen["voted_hit_tail"]
    assert moving["updates"] > 100 and moving["wrong_updates"] < 0.02 * moving["updates"]
    scores = {k: np.array([frozen[k], moving[k]]) for k in T.TRACK_SCORE_KEYS}
    assert T.pick_tracker(scores) == 1 and T.pick_tracker(scores, max_wrong_rate=0.0) == 0


def test_settings_are_checked():
    emb, exp, rows, ids = stream(n=5)
    for bad in (dict(rate=1.0), dict(rate=-0.1), dict(rate=float("nan")), dict(vote=0), dict(vote=257), dict(vote=True),
                dict(min_cosine=float("nan")), dict(dwell=3)):
        with pytest.raises(ValueError):
            track_reference(emb, rows, ids, **bad)
    with pytest.raises(ValueError):
        track_reference(emb, rows, ids[::-1])
    with pytest.raises(ValueError):
        track_reference(emb, rows[:-1], ids)
    assert T.track_grid(rate=[0.0, 0.1], agree=[False, True])[1] == dict(rate=0.0, agree=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "contrastiveprosthetics_amd", "csrc")], check=True)
    from contrastiveprosthetics_amd import _lib
    return _lib.load()


def declaration(hdr, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_declared_exported_and_bound_and_the_old_pushes_unchanged(lib):
    from contrastiveprosthetics_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(LIB)
    for n in EMBED + TRACK:
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
        assert len(declaration(hdr, n)) == len(_lib.SYMBOLS[n][1]), n
    # an embed entry is the mapped entry plus `float* embeddings` in front of the stream; the eight older entries are as they were
    single = ["const cp_online_config* cfg", "void* ws", "size_t ws_bytes", "const float* raw", "int64_t n_samples", "const float* mean_std"]
    multi = ["const cp_online_config* cfg", "int32_t n_streams", "int32_t max_rows", "void* ws", "size_t ws_bytes", "const float* raw",
             "const int32_t* counts", "int64_t total_samples", "int32_t total_windows", "const float* mean_std"]
    cmap = ["const int32_t* map_src", "const float* map_fill"]
    outs = ["int32_t* pred", "int32_t* voted", "float* logits", "float* windows"]
    for kind, head in (("cp_online", single), ("cp_online_adapt", single), ("cp_online_multi", multi), ("cp_online_multi_adapt", multi)):
        assert declaration(hdr, kind + "_push") == head + outs + ["void* stream"]
        assert declaration(hdr, kind + "_push_mapped") == head + cmap + outs + ["void* stream"]
        assert declaration(hdr, kind + "_push_embed") == head + cmap + outs + ["float* embeddings", "void* stream"]
        assert _lib.SYMBOLS[kind + "_push_embed"][1][:-2] == _lib.SYMBOLS[kind + "_push_mapped"][1][:-1]
    body = hdr[hdr.index("typedef struct cp_online_track_config {"):hdr.index("} cp_online_track_config;")]
    fields = re.findall(r"\b(?:int32_t|float|double)\s+(\w+);", body)
    assert fields == [f[0] for f in _lib.cp_online_track_config._fields_]
    assert ctypes.sizeof(_lib.cp_online_track_config) == 32 and _lib.cp_online_track_config.rate.offset == 8


def test_workspace_is_per_stream_state(lib):
    one = lib.cp_online_track_workspace_bytes(1)
    # K, head, len, ids[64], ring[256], two int64 counters, anchor and rows [64][16] f32, acc [64][16] f64
    assert one >= 4 * (3 + 64 + 256) + 2 * 8 * 64 + 2 * 4 * 64 * 16 + 8 * 64 * 16 and one % 256 == 0
    sizes = [lib.cp_online_track_workspace_bytes(s) for s in (1, 2, 64, 256)]
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3] <= 256 * one
    assert lib.cp_online_track_workspace_bytes(0) == one
    assert T._OT_WORDS * 4 * 256 <= sizes[3] < T._OT_WORDS * 4 * 256 + 256       # PrototypeTracker.state reads this layout


def _tcfg(**kw):
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_track_config()
    cfg.vote, cfg.agree, cfg.rate, cfg.min_cosine, cfg.min_margin, cfg.min_anchor_cosine = 25, 1, 0.05, 0.5, 0.05, 0.7
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    """host memory as the 'workspace': every refusal returns before a launch, which on this machine would fail differently"""
    S = 4
    need = lib.cp_online_track_workspace_bytes(S)
    buf = ctypes.create_string_buffer(need + 256)
    ws = (ctypes.addressof(buf) + 255) // 256 * 256
    ids = (ctypes.c_int32 * 65)(*range(65))
    fbuf = ctypes.create_string_buffer(64 * 16 * 4 + 64)
    rows_p = (ctypes.addressof(fbuf) + 15) // 16 * 16
    cnt = (ctypes.c_int32 * S)()
    out = (ctypes.c_int32 * 8)()
    big = ctypes.create_string_buffer(64 * 16 * 8)
    bigp = (ctypes.addressof(big) + 7) // 8 * 8

    def calls(cfg, n_streams=S, w=ws, nbytes=need):
        cr = ctypes.byref(cfg)
        return (("cp_online_track_set_rows", lambda: lib.cp_online_track_set_rows(cr, n_streams, w, nbytes, 0, ids, rows_p, 2, None)),
                ("cp_online_track_reset", lambda: lib.cp_online_track_reset(cr, n_streams, w, nbytes, -1, 0, None)),
                ("cp_online_track_push", lambda: lib.cp_online_track_push(cr, n_streams, w, nbytes, rows_p, cnt, cnt, 1, out, out, None,
                                                                          64, out, None)),
                ("cp_online_track_rows", lambda: lib.cp_online_track_rows(cr, n_streams, w, nbytes, 0, rows_p, bigp, bigp, None)))

    def err(rc, entry, what):
        assert rc == ERR_ARG, (entry, what, rc)
        msg = lib.cp_last_error()
        assert entry.encode() in msg and what.encode() in msg, msg

    def each(cfg, what, **kw):                      # every entry refuses, one at a time (cp_last_error is the last call's)
        for entry, call in calls(cfg, **kw):
            err(call(), entry, what)

    each(_tcfg(vote=0), "vote")
    each(_tcfg(vote=257), "vote")
    each(_tcfg(rate=1.0), "rate")                                          # beta = 1
    each(_tcfg(rate=-0.01), "rate")
    each(_tcfg(rate=float("nan")), "rate")
    each(_tcfg(agree=2), "agree")
    each(_tcfg(min_cosine=float("nan")), "NaN")
    each(_tcfg(min_anchor_cosine=float("nan")), "NaN")
    each(_tcfg(), "n_streams", n_streams=0)
    each(_tcfg(), "n_streams", n_streams=257)
    each(_tcfg(), "workspace", w=None)
    each(_tcfg(), "workspace", w=ws + 4)
    each(_tcfg(), "workspace", nbytes=need - 257)                          # a short workspace
    each(_tcfg(), "workspace", n_streams=S + 1)                            # sized for fewer streams
    cfg = _tcfg()
    cr = ctypes.byref(cfg)
    sr, rs, pu, ro, sw = TRACK[1:]
    err(lib.cp_online_track_set_rows(None, S, ws, need, 0, ids, rows_p, 2, None), sr, "config")
    err(lib.cp_online_track_set_rows(cr, S, ws, need, 0, ids, rows_p, 0, None), sr, "classes")             # K = 0
    err(lib.cp_online_track_set_rows(cr, S, ws, need, 0, ids, rows_p, 65, None), sr, "classes")            # K = 65
    err(lib.cp_online_track_set_rows(cr, S, ws, need, 0, None, rows_p, 2, None), sr, "classes")
    err(lib.cp_online_track_set_rows(cr, S, ws, need, 0, ids, None, 2, None), sr, "classes")
    err(lib.cp_online_track_set_rows(cr, S, ws, need, S, ids, rows_p, 2, None), sr, "stream index")
    err(lib.cp_online_track_set_rows(cr, S, ws, need, -1, ids, rows_p, 2, None), sr, "stream index")
    err(lib.cp_online_track_set_rows(cr, S, ws, need, 0, ids, rows_p + 2, 2, None), sr, "misaligned")
    for bad in ([3, 2], [2, 2], [-1, 4], [0, 2 ** 31 - 1]):               # unsorted, repeated, negative (-1 is 'none'), too large
        err(lib.cp_online_track_set_rows(cr, S, ws, need, 0, (ctypes.c_int32 * 2)(*bad), rows_p, 2, None), sr, "ascending")
    err(lib.cp_online_track_reset(cr, S, ws, need, S, 0, None), rs, "stream index")
    err(lib.cp_online_track_reset(cr, S, ws, need, -2, 0, None), rs, "stream index")
    err(lib.cp_online_track_reset(cr, S, ws, need, 0, 2, None), rs, "what")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p, cnt, cnt, -1, out, out, None, 64, out, None), pu, "total_rows")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p, cnt, cnt, 65537, out, out, None, 64, out, None), pu, "total_rows")
    err(lib.cp_online_track_push(cr, S, ws, need, None, cnt, cnt, 1, out, out, None, 64, out, None), pu, "required")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p, None, cnt, 1, out, out, None, 64, out, None), pu, "required")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p, cnt, cnt, 1, None, out, None, 64, out, None), pu, "required")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p, cnt, cnt, 1, out, out, None, 64, None, None), pu, "required")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p, cnt, cnt, 1, out, out, rows_p, 0, out, None), pu, "ldl")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p + 4, cnt, cnt, 1, out, out, None, 64, out, None), pu, "16-byte")
    err(lib.cp_online_track_push(cr, S, ws, need, rows_p, cnt, cnt, 1, ctypes.addressof(out) + 2, out, None, 64, out, None), pu,
        "misaligned")
    assert lib.cp_online_track_push(cr, S, ws, need, None, None, None, 0, None, None, None, 0, None, None) == 0     # no rows: nothing to do
    err(lib.cp_online_track_rows(cr, S, ws, need, S, rows_p, bigp, bigp, None), ro, "stream index")
    err(lib.cp_online_track_rows(cr, S, ws, need, 0, rows_p + 2, bigp, bigp, None), ro, "misaligned")
    err(lib.cp_online_track_rows(cr, S, ws, need, 0, rows_p, bigp + 4, bigp, None), ro, "misaligned")

    def sweep(emb=rows_p, n_rows=8, k=2, rows=rows_p, exp=cnt, tail=0, cfgs=bigp, g=1, scores=bigp, pred=None):
        return lib.cp_online_track_sweep(emb, n_rows, k, rows, exp, tail, cfgs, g, scores, pred, None, None, None)

    err(sweep(k=0), sw, "n_classes")
    err(sweep(k=65), sw, "n_classes")
    err(sweep(g=0), sw, "n_configs")
    err(sweep(g=65537), sw, "n_configs")
    err(sweep(n_rows=0), sw, "n_rows")
    err(sweep(n_rows=2 ** 31), sw, "n_rows")
    err(sweep(tail=-1), sw, "tail_from")
    for missing in ("emb", "rows", "exp", "cfgs", "scores"):
        err(sweep(**{missing: None}), sw, "required")
    err(sweep(emb=rows_p + 4), sw, "16-byte")
    err(sweep(cfgs=bigp + 4), sw, "misaligned")
    err(sweep(scores=bigp + 4), sw, "misaligned")
    err(sweep(pred=ctypes.addressof(out) + 2), sw, "misaligned")


def test_embed_entries_refuse_as_the_mapped_pushes_do(lib):
    """the new push entries run the checks of the entries they extend, under their own names, and refuse a misaligned
    destination before anything is enqueued"""
    from contrastiveprosthetics_amd import _lib
    cfg = _lib.cp_online_config()
    cfg.dtype, cfg.max_windows, cfg.vote, cfg.phase, cfg.n_coef = 0, 16, 25, 0, 3
    cfg.a[0] = 1.0
    need = max(lib.cp_online_workspace_bytes(16, 0), lib.cp_online_adapt_workspace_bytes(16, 0),
               lib.cp_online_multi_workspace_bytes(2, 16, 0), lib.cp_online_multi_adapt_workspace_bytes(2, 16, 0))
    buf = ctypes.create_string_buffer(need + 256)
    ws = (ctypes.addressof(buf) + 255) // 256 * 256
    raw = ctypes.create_string_buffer(20 * 12 * 4 + 16)
    rawp = (ctypes.addressof(raw) + 15) // 16 * 16
    out = (ctypes.c_int32 * 64)()
    cr = ctypes.byref(cfg)
    for name in ("cp_online_push_embed", "cp_online_adapt_push_embed"):
        fn = getattr(lib, name)
        assert fn(cr, ws, need, rawp, 20, rawp, None, None, out, out, None, None, rawp + 2, None) == ERR_ARG
        assert name.encode() in lib.cp_last_error() and b"embeddings" in lib.cp_last_error()
        assert fn(cr, ws, need, None, 20, rawp, None, None, out, out, None, None, rawp, None) == ERR_ARG
        assert name.encode() in lib.cp_last_error()
        assert fn(cr, ws, need, rawp, 0, rawp, None, None, out, out, None, None, rawp, None) == 0          # an empty push
    for name in ("cp_online_multi_push_embed", "cp_online_multi_adapt_push_embed"):
        fn = getattr(lib, name)
        assert fn(cr, 2, 16, ws, need, rawp, out, 20, 1, rawp, None, None, out, out, None, None, rawp + 2, None) == ERR_ARG
        assert name.encode() in lib.cp_last_error() and b"embeddings" in lib.cp_last_error()
        assert fn(cr, 2, 16, ws, need, rawp, None, 20, 1, rawp, None, None, out, out, None, None, rawp, None) == ERR_ARG
        assert name.encode() in lib.cp_last_error()
        assert fn(cr, 2, 16, ws, need, rawp, out, 0, 0, rawp, None, None, out, out, None, None, rawp, None) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper, without a device
# ---------------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_bad_settings_and_is_exported_lazily():
    import contrastiveprosthetics_amd as cp

    class Dec:
        class_ids, n_seen, vote, ws, device = None, 0, 25, None, None

        def push(self, *a, **k):
            raise AssertionError("not pushed")

    assert cp.PrototypeTracker is T.PrototypeTracker and cp.track_reference is track_reference and cp.sweep_tracker is T.sweep_tracker
    assert cp.pick_tracker is T.pick_tracker and cp.embed_recording is T.embed_recording
    t = T.PrototypeTracker(Dec(), rate=0.02)
    assert t.vote == 25 and t.settings["rate"] == 0.02 and t._cfg.agree == 1
    t.set(rate=0.0, agree=False)
    assert t._cfg.rate == 0.0 and t._cfg.agree == 0
    for bad in (dict(rate=1.0), dict(vote=9), dict(min_margin=float("nan")), dict(release=1)):
        with pytest.raises(ValueError):
            t.set(**bad)
    assert t._cfg.rate == 0.0                                          # nothing changed
    with pytest.raises(ValueError):
        t.use(dict(vote=9))
    t.use(dict(vote=25, rate=0.1))
    assert t._cfg.rate == 0.1
    with pytest.raises(ValueError):
        T.PrototypeTracker(Dec(), vote=300)
    with pytest.raises(TypeError):
        T.PrototypeTracker(object())
    with pytest.raises(ValueError):
        T.sweep_tracker(None, [], [0, 1], np.zeros((2, 16), F), [])     # no configs
    with pytest.raises(ValueError):
        T.sweep_tracker(None, [], [0, 1], np.zeros((2, 16), F), [dict(rate=2.0)])
