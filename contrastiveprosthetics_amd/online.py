"""Online grasp decoding: a live raw sEMG stream -> a predicted and a voted grasp every 10 ms.

The reference exists for this use (README.md:11-19): a prosthetic hand reads the sEMG of the forearm as it arrives, the user
keeps the subset of grasps that makes sense at the moment, and the model reports a grasp every 10 ms, voted over the last
250 ms (code/constants.py:74-78: 25 windows at 100 Hz).  `OnlineDecoder` does that on the MI355X through the cp_online_*
entries of include/cpnative.h (csrc/online.cuh):

* the front end is the per-sample transform of `preprocess_segments` + `normalize_` with its state (IIR, RMS history, sample
  count) kept in the decoder's workspace between pushes: a recording pushed in any chunking yields the windows
  `normalize_(preprocess_segments(r[None], keep=phase + 20 * arange(K)), mean, std)` bit for bit;
* the encoder is the eval-mode sEMG encoder with running-statistics BatchNorm folded into the weights (f32 or bf16);
* the class table holds K <= 64 rows (one-hot class ids, glove rows through the glove encoder, or raw embeddings), the
  prediction is the argmax of z/|z| . E/|E| (first maximum), the vote the mode of the last `vote` predictions (ties: smallest id).

`adapt=alpha` builds the adaptive form (cp_online_adapt_*, csrc/online_adapt.cuh): BatchNorm stays unfolded, its float64
statistics live in the workspace, `calibrate()` sets them from a recording (AdaBN: the reference's default model, which the
folded form cannot run), and every push can track the stream with rate alpha per window (0: frozen).

`MultiStreamDecoder` decodes up to 256 streams through one model in one chain of launches per push (cp_online_multi_*,
csrc/online_multi.cuh): the folded weights once, each stream's state and class table of its own, and every stream's outputs
bit-identical to those of its own `OnlineDecoder`.  `AdaptiveMultiStreamDecoder` is its adaptive form (cp_online_multi_adapt_*,
csrc/online_multi_adapt.cuh): per stream float64 BatchNorm statistics, calibration and alpha, each stream bit-identical to its
own `OnlineDecoder(adapt=alpha)`.

`CommandGate` wraps any of the four decoders and turns the logits of every push into a command a hand can follow, on the
device (cp_online_gate_*, csrc/online_gate.cuh): rejection by cosine threshold and margin, a weighted vote ring, a dwell time
before a new grasp and a release time before none.  `sweep_gate` chooses its settings: it runs many of them over the logits
of a cued recording in one pass on the device (cp_online_gate_sweep) and returns each one's score against the cues
(`expected_commands`, `score_commands`, `pick_gate`).  `search_grasp_sets` answers the question before that one, which grasps
to keep: it scores many class subsets of the same recording in one pass on the device (`sweep_subsets`,
cp_online_subset_sweep, csrc/online_subsets.cuh) as the decoders would decode it with that subset alone (`score_subset` is the
definition), all subsets of a size where that is affordable and a beam beyond, and ranks them (`rank_subsets`).

`GraspDrive` adds what a hand needs besides the class: a proportional level per window from the normalised windows the
decoders already emit, and the health of every electrode, on the device behind a gate or a decoder (cp_online_drive_*,
csrc/online_drive.cuh); `drive_profile` makes its profile from the cued recording enrolment already has.

`set_channel_map` tells a decoder which physical electrode feeds each model channel, or that a channel is masked (a sleeve
that went back on rotated, a dead electrode): the front end reads the map in its own launch (cp_online_*_mapped), and
everything behind it -- encoder, gate, drive, enrolment, calibration -- sees model channels.  `score_channel_maps` finds the
map: it scores many candidates (`rotations`, `leave_one_out`) over a cued recording in one pass on the device
(cp_online_*map_sweep, csrc/online_maps.cuh) exactly as fresh mapped decoders would decode it, and `pick_channel_map` takes
the best.

`finetune` is the gradient step of the personalisation chain (calibrate -> enroll -> fine-tune -> sweep the gate): the
projection and the class rows behind the shared encoder are trained on the device with the model's own loss on the user's cued
recording (cp_online_finetune_*, csrc/online_finetune.cuh; `finetune.finetune_reference` is the definition), and
`projection` / `set_projection` / `reset_projection` store, restore and drop the user's head.  The multi-stream decoders share
one projection among their streams unless they are built with `stream_projections=True`: then each stream has a slot of its
own in a projection bank next to the workspace (cp_online_projections_*, the *_proj entries, csrc/online_projections.cuh),
`set_projection(stream, W, b)`, `finetune(stream, ..., train_projection=True)` and `Readout.install(decoder, stream=)` fill
it, and push, `enroll` and `score_channel_maps` of that stream decode with it, bit for bit as the stream's own
`OnlineDecoder` with the same projection set; the launches per push do not change.

`realign.realign_cues` stands in front of that chain: a user's cue runs ahead of the movement, and it moves the labels of a
cued recording onto the onset and offset the sEMG itself shows, on the device and without the model (cp_online_realign*,
csrc/online_realign.cuh; `realign.realign_reference` is the definition, `realign.sample_labels` gives `enroll` and `finetune`
their per-sample labels).

`push(..., return_embeddings=True)` also gives out z / |z| of every window (cp_online_*_push_embed), which is what
`track.PrototypeTracker` reads: class rows that follow the user's drifting embeddings between enrolments, on the device behind
any of the four decoders (cp_online_track_*, csrc/online_track.cuh; `track.track_reference` is the definition).

The number of windows a push emits follows from sample counts alone (`windows_emitted`), so a push never waits for the device:
its outputs are device tensors on torch's current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import CP_BF16, CP_D_E, CP_F32, CP_FP8, CP_TASKS
from .constants import EMG_DIM, RMS_WINDOW, WINDOW_EDGE
from .engine import Engine
from .preprocess import butter_bandpass

STRIDE = _lib.CP_ONLINE_STRIDE          # raw samples per window: 2 kHz -> 100 Hz
VOTE = 25                               # code/constants.py:74-78: 250 ms at 100 Hz
MAX_CLASSES = _lib.CP_ONLINE_MAX_CLASSES


def windows_before(n_samples: int, phase: int = 0) -> int:
    """Windows final once `n_samples` raw samples have arrived: window k sits at RMS-series position phase + 20 k, which
    belongs to raw sample phase + 20 k + WINDOW_EDGE and needs WINDOW_EDGE samples after it, i.e. raw sample phase + 20 k + 10."""
    return max(0, (n_samples - phase - 2 * WINDOW_EDGE - 1 + STRIDE) // STRIDE)


def windows_emitted(n_seen: int, n: int, phase: int = 0) -> int:
    """Windows a push of `n` samples emits after `n_seen` samples since the last reset."""
    return windows_before(n_seen + n, phase) - windows_before(n_seen, phase)


def _engine_of(model_or_engine, who: str = "OnlineDecoder") -> Engine:
    e = getattr(model_or_engine, "engine", model_or_engine)
    if not isinstance(e, Engine):
        raise TypeError(f"{who} takes a contrastiveprosthetics_amd Model or Engine")
    return e


def _check_settings(e: Engine, dtype, vote, phase, max_windows_per_push, who: str) -> str:
    """The settings every online decoder checks before it allocates anything; returns the dtype name."""
    if dtype is None:
        dtype = {CP_F32: "f32", CP_BF16: "bf16", CP_FP8: "fp8"}[e.dtype]
    if dtype == "fp8":
        raise _lib.CpNativeError(f"{who} runs in 'f32' or 'bf16'; there is no 8-bit online path")
    if dtype not in ("f32", "bf16"):
        raise ValueError("dtype must be 'f32' or 'bf16'")
    if e.specs["emg_net.last.0.weight"][0] != CP_D_E:
        raise _lib.CpNativeError(f"{who} is built for d_e={CP_D_E}")
    if not 1 <= int(vote) <= _lib.CP_ONLINE_MAX_VOTE:
        raise ValueError(f"vote must lie in 1..{_lib.CP_ONLINE_MAX_VOTE}")
    if not 0 <= int(phase) < STRIDE:
        raise ValueError(f"phase must lie in 0..{STRIDE - 1}")
    if not 1 <= int(max_windows_per_push) <= _lib.CP_ONLINE_MAX_WINDOWS:
        raise ValueError(f"max_windows_per_push must lie in 1..{_lib.CP_ONLINE_MAX_WINDOWS}")
    return dtype


def _filter(b, a):
    if b is None:
        b, a = butter_bandpass()
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if len(b) != len(a) or not 2 <= len(b) <= 17 or a[0] == 0.0:
        raise ValueError("b and a: 2..17 coefficients each, a[0] != 0")
    return b, a


def _config(dtype: str, max_windows: int, vote: int, phase: int, b, a):
    cfg = _lib.cp_online_config()
    cfg.dtype = CP_F32 if dtype == "f32" else CP_BF16
    cfg.max_windows = max_windows
    cfg.vote = vote
    cfg.phase = phase
    cfg.n_coef = len(b)
    for i in range(len(b)):
        cfg.b[i], cfg.a[i] = float(b[i]), float(a[i])
    return cfg


def _channels(v, device) -> torch.Tensor:
    t = torch.as_tensor(v, dtype=torch.float32).to(device).reshape(-1)
    if t.numel() == 1:
        t = t.expand(EMG_DIM)
    if t.numel() != EMG_DIM:
        raise ValueError("mean and std: one value or one per channel (12)")
    return t


def _check_count(k: int):
    if k < 1:
        raise ValueError("the class list is empty")
    if k > MAX_CLASSES:
        raise ValueError(f"at most {MAX_CLASSES} classes, got {k}")


def _check_raw(t, what: str = "raw"):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or t.dim() != 2 \
            or t.shape[1] != EMG_DIM:
        raise ValueError(f"{what} must be an (n, 12) float32 tensor on the GPU")


def _check_map(src, fill=None):
    """An electrode map as `set_channel_map` takes it -> (src (12,) int32, fill (12,) float32) numpy arrays, or None for
    src=None.  src[d] in -1..11: the physical channel that feeds model channel d, -1 masked; fill: one value or 12, finite."""
    if src is None:
        if fill is not None:
            raise ValueError("fill goes with a map: src=None clears the map")
        return None
    a = np.asarray(src)
    if a.ndim != 1 or a.shape[0] != EMG_DIM:
        raise ValueError(f"src must hold {EMG_DIM} entries: the physical channel of each model channel, or -1")
    if a.dtype.kind not in "iu":
        raise ValueError("src must be integers")
    a = a.astype(np.int64)
    if a.min() < -1 or a.max() >= EMG_DIM:
        raise ValueError(f"src must lie in -1..{EMG_DIM - 1}")
    f = np.zeros(EMG_DIM, dtype=np.float32) if fill is None else np.asarray(fill, dtype=np.float32).reshape(-1)
    if f.shape[0] == 1:
        f = np.repeat(f, EMG_DIM)
    if f.shape[0] != EMG_DIM:
        raise ValueError(f"fill: one value or one per model channel ({EMG_DIM})")
    if not np.isfinite(f).all():
        raise ValueError("fill must be finite")
    return a.astype(np.int32), f.astype(np.float32)


def _map_on_device(m, device):
    """(src, fill) of `_check_map` as one (12,) int32 and one (12,) float32 device tensor"""
    return torch.as_tensor(m[0]).to(device), torch.as_tensor(m[1]).to(device)


def _map_windows(w: torch.Tensor, m) -> torch.Tensor:
    """the masked columns of the windows w (K, 12) overwritten with the map's fill"""
    masked = np.nonzero(m[0] < 0)[0]
    if masked.size:
        w[:, torch.as_tensor(masked, device=w.device)] = torch.as_tensor(m[1][masked], device=w.device)
    return w


def _check_projection(W, b):
    """(W (16, 512), b (16,)) as f32 tensors where they are; a wrong shape or a value that is not finite is a ValueError"""
    W, b = torch.as_tensor(W, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    if tuple(W.shape) != (CP_D_E, 512) or tuple(b.shape) != (CP_D_E,):
        raise ValueError(f"W must be ({CP_D_E}, 512) and b ({CP_D_E},)")
    if not (bool(torch.isfinite(W).all()) and bool(torch.isfinite(b).all())):
        raise ValueError("W and b must be finite")
    return W, b


def _tail_view(dec, n_streams: int, max_rows: int, rows: int, adaptive: bool, multi: bool) -> torch.Tensor:
    """the block of a decoder's workspace that holds the tail inputs of its last push, as a (rows, 512) view"""
    off = dec.lib.cp_online_tail_offset(C.byref(dec._cfg), n_streams, max_rows, int(adaptive), int(multi))
    if off == 0:
        raise _lib.CpNativeError("cp_online_tail_offset failed: " + dec.lib.cp_last_error().decode("utf-8", "replace"))
    dt = torch.float32 if dec.dtype == "f32" else torch.bfloat16
    return dec.ws[off:off + rows * 512 * (4 if dec.dtype == "f32" else 2)].view(dt).view(rows, 512)


class _OnStream:
    """a decoder or gate on `self.device`: its C entries run on torch's current stream there"""

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream


def _class_table(e: Engine, classes=None, glove=None, table=None, ids=None):
    """The class table of `set_classes` (see OnlineDecoder.set_classes): (K, 16) f32 rows on the device, sorted by id, and the
    sorted ids (K,) int64.  Raises before anything is enqueued on a decoder."""
    if sum(x is not None for x in (classes, glove, table)) != 1:
        raise ValueError("set_classes takes exactly one of classes, glove, table")
    if glove is not None and e.adabn:
        raise _lib.CpNativeError("glove class rows need a glove encoder with running statistics: on an AdaBN model its "
                                 "batch statistics would come from a zero-padded group; pass classes= or table=")
    if classes is not None:
        cid = torch.as_tensor(np.asarray(classes, dtype=np.int64).reshape(-1))
        _check_count(cid.numel())
        if int(cid.min()) < 0 or int(cid.max()) >= CP_TASKS:
            raise ValueError(f"class ids must lie in 0..{CP_TASKS - 1}")
        ids_t = cid
        rows = None
    else:
        src = glove if glove is not None else table
        width = 20 if glove is not None else CP_D_E
        src = torch.as_tensor(src, dtype=torch.float32)
        if src.dim() != 2 or src.shape[1] != width:
            raise ValueError(f"{'glove' if glove is not None else 'table'} must be (K, {width})")
        _check_count(src.shape[0])
        ids_t = torch.arange(src.shape[0]) if ids is None else torch.as_tensor(np.asarray(ids, dtype=np.int64).reshape(-1))
        if ids_t.numel() != src.shape[0]:
            raise ValueError("one id per row")
        rows = src
    if len(set(ids_t.tolist())) != ids_t.numel():
        raise ValueError("class ids must be distinct")
    device = e.device
    order = torch.argsort(ids_t)
    ids_t = ids_t[order]
    if rows is None:
        w, b = e.values.views["glove_net.easy.0.weight"], e.values.views["glove_net.easy.0.bias"]
        tab = (w[:, ids_t.to(device)].t() + b).contiguous()
    elif glove is not None:
        k = rows.shape[0]
        padded = torch.zeros((k + CP_TASKS - 1) // CP_TASKS * CP_TASKS, 20)     # the glove encoder takes whole groups of 41 rows
        padded[:k] = rows[order]
        zg = e.glove_forward(padded.to(device).reshape(1, -1, 20), training=False)
        tab = zg[:k].contiguous()
    else:
        tab = rows[order].to(device).contiguous()
    return tab.to(torch.float32).contiguous(), ids_t


def _calibration_windows(raw: torch.Tensor, b, a, phase: int, mean_std: torch.Tensor, channel_map=None) -> torch.Tensor:
    """The windows a fresh stream emits for `raw` (n, 12), by the offline path (preprocess_segments + normalize_): the whole
    recording as one segment, 256 kept positions per call.  Valid for a recording of any length: cp_preprocess_emg keeps
    its positions in 32 bits.  channel_map (src, fill of `_check_map`): the windows in model channels -- the raw columns
    permuted by src first, the masked columns overwritten with fill last."""
    from .preprocess import normalize_, preprocess_segments
    _check_raw(raw)
    if channel_map is not None:
        cols = np.where(channel_map[0] < 0, np.arange(EMG_DIM), channel_map[0])
        raw = raw[:, torch.as_tensor(cols, dtype=torch.long, device=raw.device)]
    k = windows_before(raw.shape[0], phase)
    if k < 2:
        raise ValueError("calibration takes at least 2 windows")
    raw = raw.contiguous()[None]
    keep = phase + STRIDE * np.arange(k)
    step = _lib.CP_ONLINE_MAX_WINDOWS                      # positions one call of the offline transform keeps
    w = torch.cat([preprocess_segments(raw, b=b, a=a, keep=keep[i:i + step]) for i in range(0, k, step)], dim=1)
    w = normalize_(w.contiguous(), mean_std[0], mean_std[1])[0]
    return w if channel_map is None else _map_windows(w, channel_map)


# ---------------------------------------------------------------------------------------------------------------------------
# class enrolment: per-user class rows from the user's own labelled recording (cp_online_*enroll*, csrc/online_enroll.cuh)
# ---------------------------------------------------------------------------------------------------------------------------
def window_labels(labels, phase: int = 0) -> np.ndarray:
    """The label of each window of a recording with one label per raw sample (a class id, or a negative value for "not
    labelled"; what Ninapro's `restimulus` is): window k covers the raw samples phase + 20 k .. phase + 20 k + 2 WINDOW_EDGE and
    takes their label if all 11 carry the same non-negative label, else -1.  (K,) int64 with K = windows_before(n, phase).
    Host only (numpy).  A user's own cue is not yet such a label -- the movement starts and ends behind it --
    and `realign.realign_cues` moves it onto the movement first."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.dtype.kind not in "iu":
        raise ValueError("labels must be a 1-d integer array: one class id (or a negative value) per raw sample")
    if not 0 <= int(phase) < STRIDE:
        raise ValueError(f"phase must lie in 0..{STRIDE - 1}")
    lab = lab.astype(np.int64)
    k = windows_before(lab.shape[0], int(phase))
    if k == 0:
        return np.zeros(0, dtype=np.int64)
    span = lab[(int(phase) + STRIDE * np.arange(k))[:, None] + np.arange(2 * WINDOW_EDGE + 1)]
    same = (span == span[:, :1]).all(axis=1) & (span[:, 0] >= 0)
    return np.where(same, span[:, 0], -1)


def recording_windows(raw: torch.Tensor, mean_std: torch.Tensor, b=None, a=None, phase: int = 0, channel_map=None) -> torch.Tensor:
    """The windows a fresh stream emits for `raw` (n, 12) f32 on the GPU, (K, 12) with K = windows_before(n, phase): one pass
    of the stateful front end (cp_online_windows) over the recording, bit-identical to the offline path
    (`preprocess_segments` + `normalize_`), which filters the recording again for every 256 positions it keeps.  mean_std
    (2, 12) f32 on the GPU.  channel_map: None, or (src, fill) as `set_channel_map` takes them -- the windows in model
    channels, as a decoder with that map emits them (cp_online_windows_mapped)."""
    _check_raw(raw)
    cmap = None if channel_map is None else _check_map(*channel_map)
    if not 0 <= int(phase) < STRIDE:
        raise ValueError(f"phase must lie in 0..{STRIDE - 1}")
    b, a = _filter(b, a)
    lib = _lib.load()
    cfg = _config("f32", _lib.CP_ONLINE_MAX_WINDOWS, 1, int(phase), b, a)
    raw = raw.contiguous()
    mean_std = mean_std.to(device=raw.device, dtype=torch.float32).contiguous()
    if tuple(mean_std.shape) != (2, EMG_DIM):
        raise ValueError("mean_std must be (2, 12)")
    n = raw.shape[0]
    out = torch.empty(max(windows_before(n, phase), 1), EMG_DIM, dtype=torch.float32, device=raw.device)
    state = torch.zeros(lib.cp_online_frontend_state_bytes(), dtype=torch.uint8, device=raw.device)
    stream = torch.cuda.current_stream(raw.device).cuda_stream
    step = STRIDE * _lib.CP_ONLINE_MAX_WINDOWS
    dev_map = None if cmap is None else _map_on_device(cmap, raw.device)
    for s in range(0, n, step):
        m = min(step, n - s)
        row = windows_before(s, phase)                         # 20 W samples complete at most W windows: out has the room
        dst = out[row:].data_ptr() if row < out.shape[0] else out.data_ptr()
        if dev_map is None:
            _lib.check(lib.cp_online_windows(C.byref(cfg), state.data_ptr(), state.numel(), raw[s:].data_ptr(), m, mean_std.data_ptr(),
                                             dst, stream), "cp_online_windows")
        else:
            _lib.check(lib.cp_online_windows_mapped(C.byref(cfg), state.data_ptr(), state.numel(), raw[s:].data_ptr(), m,
                                                    mean_std.data_ptr(), dev_map[0].data_ptr(), dev_map[1].data_ptr(), dst, stream),
                       "cp_online_windows_mapped")
    return out[:windows_before(n, phase)]


class _Enrolment:
    """the accumulator of one decoder (or stream): acc (64, 17) float64 on the device, laid out by `ids` (ascending), and the
    window counts per slot as the host knows them"""

    def __init__(self, ids: np.ndarray, device):
        self.ids = ids.astype(np.int64)
        self.counts = np.zeros(ids.shape[0], dtype=np.int64)
        self.acc = torch.zeros(MAX_CLASSES, 17, dtype=torch.float64, device=device)


def _sample_labels(labels, n: int) -> np.ndarray:
    if isinstance(labels, torch.Tensor):
        if labels.is_floating_point() or labels.dtype == torch.bool:
            raise ValueError("labels must be integers: one class id (or a negative value) per raw sample")
        labels = labels.detach().cpu().numpy()
    lab = np.asarray(labels)
    if lab.dtype.kind not in "iu":
        raise ValueError("labels must be integers: one class id (or a negative value) per raw sample")
    if lab.ndim != 1 or lab.shape[0] != n:
        raise ValueError(f"labels must hold one entry per raw sample ({n}), got shape {tuple(lab.shape)}")
    return lab.astype(np.int64)


class _EnrollMixin(_OnStream):
    """`enroll` of the online decoders.  `key` is None (OnlineDecoder) or a stream index; a decoder supplies _enroll_view,
    _enroll_call and _enroll_install."""

    def _enroll(self, key, raw, labels, mix, min_windows, add, accumulate):
        ids_cur, prior, calibrated = self._enroll_view(key)
        if ids_cur is None:
            raise _lib.CpNativeError("enroll() needs a class table: set_classes() first (it is the prior and the id list)")
        if not calibrated:
            raise _lib.CpNativeError("an AdaBN model has no BatchNorm statistics: calibrate() first, then enroll()")
        if not 0.0 <= float(mix) <= 1.0:
            raise ValueError("mix must lie in [0, 1]")
        if int(min_windows) < 1:
            raise ValueError("min_windows must be at least 1")
        _check_raw(raw)
        wl = window_labels(_sample_labels(labels, raw.shape[0]), self.phase)
        keep = np.nonzero(wl >= 0)[0]
        if keep.size == 0:
            raise ValueError("the recording has no labelled window: a window needs 11 samples in a row of one non-negative label")
        rec = self._enroll_rec.get(key)
        old_ids = rec.ids if rec is not None else ids_cur
        new = np.setdiff1d(np.unique(wl[keep]), old_ids)
        if new.size and not add:
            raise ValueError(f"labels hold class ids the decoder does not have: {new.tolist()} (add=True enrols them as new classes)")
        ids = np.union1d(old_ids, new)
        if ids.size > MAX_CLASSES:
            raise ValueError(f"at most {MAX_CLASSES} classes, got {ids.size}")
        if int(ids.max()) >= 2 ** 31:
            raise ValueError("class ids must fit int32")
        counts = np.zeros(ids.size, dtype=np.int64)
        if rec is not None:
            counts[np.searchsorted(ids, rec.ids)] = rec.counts
        slots = np.searchsorted(ids, wl[keep])
        counts += np.bincount(slots, minlength=ids.size)
        if not accumulate:
            short = [int(i) for i, c in zip(ids, counts) if i not in set(ids_cur.tolist()) and c < int(min_windows)]
            if short:
                raise ValueError(f"new classes {short} have fewer than min_windows={int(min_windows)} windows: a new class has no "
                                 "prior row to fall back on")
        # ---- everything is checked: from here on work is enqueued
        if rec is None:
            rec = _Enrolment(ids, self.device)
        elif ids.size != rec.ids.size:                       # new classes: the slots of the old ones move
            acc = torch.zeros_like(rec.acc)
            acc[torch.as_tensor(np.searchsorted(ids, rec.ids), device=self.device)] = rec.acc[:rec.ids.size]
            rec.acc, rec.ids = acc, ids
        rec.counts = counts
        self._enroll_rec[key] = rec
        w = recording_windows(raw, self.mean_std, self._b, self._a, self.phase, channel_map=self._map_of(key))
        w = w[torch.as_tensor(keep, device=self.device)].contiguous()
        slots_dev = torch.as_tensor(slots.astype(np.int32), device=self.device)
        scratch = torch.empty(self.lib.cp_online_enroll_scratch_bytes(w.shape[0], self._cfg.dtype), dtype=torch.uint8, device=self.device)
        self._enroll_call(key, w.data_ptr(), int(w.shape[0]), slots_dev.data_ptr(), int(ids.size), rec.acc.data_ptr(),
                          scratch.data_ptr(), scratch.numel())
        out = {int(i): int(c) for i, c in zip(ids, counts)}
        if accumulate:
            return out
        full = torch.zeros(ids.size, CP_D_E, dtype=torch.float32, device=self.device)       # a zero row: no prior (a new class)
        full[torch.as_tensor(np.searchsorted(ids, ids_cur), device=self.device)] = prior
        table = torch.empty_like(full)
        _lib.check(self.lib.cp_online_enroll_table(rec.acc.data_ptr(), int(ids.size), full.data_ptr(), C.c_double(float(mix)),
                                                   int(min_windows), table.data_ptr(), self._stream()), "cp_online_enroll_table")
        self._enroll_install(key, table, ids)                  # (set_classes drops the accumulator: it is kept across this one)
        self._enroll_rec[key] = rec
        return out

    # ------------------------------------------------------------------ head fine-tuning (cp_online_finetune_*)
    _shared_projection = False                                 # the multi-stream decoders: one projection for all streams

    @staticmethod
    def _labelled_slots(wl: np.ndarray, ids: np.ndarray, min_windows):
        """what `finetune` and `readout.fit_projection` ask of a recording's window labels wl (M,), negative: not labelled ->
        (keep: the labelled windows, slots: their index into ids, counts (K,)); a label outside ids or a class with
        1..min_windows-1 windows is a ValueError"""
        keep = np.nonzero(wl >= 0)[0]
        if keep.size == 0:
            raise ValueError("the recording has no labelled window: a window needs 11 samples in a row of one non-negative label")
        new = np.setdiff1d(np.unique(wl[keep]), ids)
        if new.size:
            raise ValueError(f"labels hold class ids the decoder does not have: {new.tolist()} (enroll(add=True) adds a class)")
        slots = np.searchsorted(ids, wl[keep])
        counts = np.bincount(slots, minlength=ids.size)
        short = [int(i) for i, c in zip(ids, counts) if 0 < c < int(min_windows)]
        if short:
            raise ValueError(f"classes {short} have fewer than min_windows={int(min_windows)} windows")
        return keep, slots, counts

    def _recording_tail_inputs(self, key, raw, keep: np.ndarray) -> torch.Tensor:
        """u (len(keep), 512) in the compute dtype: the tail inputs of the windows `keep` of the recording raw, a stream of its
        own read through the electrode map, embedded by the decoder's own encoder (cp_online_*tail_inputs)"""
        n = int(keep.size)
        w = recording_windows(raw, self.mean_std, self._b, self._a, self.phase, channel_map=self._map_of(key))
        w = w[torch.as_tensor(keep, device=self.device)].contiguous()
        u = torch.empty(n, 512, dtype=torch.float32 if self.dtype == "f32" else torch.bfloat16, device=self.device)
        scratch = torch.empty(self.lib.cp_online_enroll_scratch_bytes(n, self._cfg.dtype), dtype=torch.uint8, device=self.device)
        self._tail_inputs_call(key, w.data_ptr(), n, u.data_ptr(), scratch.data_ptr(), scratch.numel())
        return u

    def _finetune(self, key, raw, labels, steps, lr, lr_rows, scale, anchor, balanced, train_projection, train_rows, min_windows,
                  return_loss):
        """`finetune` of the online decoders; a decoder supplies _enroll_view, _tail_inputs_call, _projection_read and
        _finetune_install.  Every refusal comes before the first device call."""
        if train_projection and self._shared_projection:
            raise ValueError("train_projection=True: the projection is shared by all streams of a multi-stream decoder, so a "
                             "stream cannot train it; pass train_projection=False to train the stream's class rows")
        ids, table, calibrated = self._enroll_view(key)
        if ids is None:
            raise _lib.CpNativeError("finetune() needs a class table: set_classes() first (its rows are where training starts)")
        if not calibrated:
            raise _lib.CpNativeError("an AdaBN model has no BatchNorm statistics: calibrate() first, then finetune()")
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or int(steps) < 0:
            raise ValueError("steps must be an integer >= 0")
        lr_rows = lr if lr_rows is None else lr_rows
        for name, x in (("lr", lr), ("lr_rows", lr_rows), ("anchor", anchor)):
            if not (np.isfinite(float(x)) and float(x) >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0")
        if not np.isfinite(float(scale)):
            raise ValueError("scale must be finite")
        if int(min_windows) < 1:
            raise ValueError("min_windows must be at least 1")
        _check_raw(raw)
        keep, slots, counts = _EnrollMixin._labelled_slots(window_labels(_sample_labels(labels, raw.shape[0]), self.phase), ids, min_windows)
        out = {int(i): int(c) for i, c in zip(ids, counts)}
        flags = (_lib.CP_ONLINE_FINETUNE_PROJECTION if train_projection else 0) | (_lib.CP_ONLINE_FINETUNE_ROWS if train_rows else 0)
        if int(steps) == 0 or flags == 0:                      # nothing to train: the decoder stays as it is, bit for bit
            return (out, torch.zeros(0, dtype=torch.float64, device=self.device)) if return_loss else out
        # ---- everything is checked: from here on work is enqueued
        lib, n, k = self.lib, int(keep.size), int(ids.size)
        u = self._recording_tail_inputs(key, raw, keep)
        W, b = self._projection_read(key)
        E = table.to(torch.float32).contiguous()
        slots_dev = torch.as_tensor(slots.astype(np.int32), device=self.device)
        state = torch.empty(lib.cp_online_finetune_state_bytes(n, k), dtype=torch.uint8, device=self.device)
        loss = torch.empty(int(steps), dtype=torch.float64, device=self.device)
        _lib.check(lib.cp_online_finetune_init(state.data_ptr(), state.numel(), self._cfg.dtype, W.data_ptr(), b.data_ptr(), E.data_ptr(),
                                               slots_dev.data_ptr(), n, k, int(bool(balanced)), self._stream()),
                   "cp_online_finetune_init")
        _lib.check(lib.cp_online_finetune_steps(C.byref(self._cfg), state.data_ptr(), state.numel(), u.data_ptr(), n, k, int(steps),
                                                float(lr), float(lr_rows), float(scale), float(anchor), flags, loss.data_ptr(),
                                                self._stream()), "cp_online_finetune_steps")
        W2, b2, E2 = torch.empty_like(W), torch.empty_like(b), torch.empty_like(E)
        _lib.check(lib.cp_online_finetune_read(state.data_ptr(), state.numel(), n, k, W2.data_ptr(), b2.data_ptr(), E2.data_ptr(), None,
                                               self._stream()), "cp_online_finetune_read")
        self._finetune_install(key, W2 if train_projection else None, b2, E2 if train_rows else None, ids)
        return (out, loss) if return_loss else out


class OnlineDecoder(_EnrollMixin):
    """Streaming decoder over a trained model (eval mode, stock BatchNorm with running statistics).

    model_or_engine: `Model` or `Engine`; mean, std: the normalisation of the training data (`build_emg_tensor` / `emg_stats`);
    classes: see `set_classes`; vote: length of the vote ring; dtype: 'f32' | 'bf16' (default: the engine's); phase: windows at
    RMS-series positions phase + 20 k; max_windows_per_push: larger pushes are split on the host.  b, a: the IIR (default
    `butter_bandpass()`).

    The weights are folded once, here: the decoder keeps using that folded copy after an optimiser step or a
    `load_state_dict` on the model until `refresh()` folds them again.

    adapt: None (the folded form: stock BatchNorm only) or alpha in [0, 1): the adaptive form, which also takes AdaBN models.
    It starts from the running statistics (stock BatchNorm) or uncalibrated (AdaBN: `calibrate()` before the first push);
    each window then moves every BatchNorm's statistics towards its own by the fraction alpha (include/cpnative.h).
    """

    def __init__(self, model_or_engine, mean, std, classes=None, vote: int = VOTE, dtype: Optional[str] = None, phase: int = 0,
                 max_windows_per_push: int = 256, b=None, a=None, adapt: Optional[float] = None):
        e = _engine_of(model_or_engine)
        if adapt is None and e.adabn:
            raise _lib.CpNativeError("OnlineDecoder needs stock BatchNorm with running statistics: an AdaBN model normalises with "
                                     "the statistics of its batch, which a live stream of a few windows does not have "
                                     "(adapt= builds the adaptive form, which calibrates them)")
        if adapt is not None and not 0.0 <= float(adapt) < 1.0:
            raise ValueError("adapt (alpha) must lie in [0, 1)")
        dtype = _check_settings(e, dtype, vote, phase, max_windows_per_push, "OnlineDecoder")
        if classes is not None:
            _check_count(len(classes))
        b, a = _filter(b, a)
        self.engine = e
        self.adapt = None if adapt is None else float(adapt)
        self.calibrated = adapt is None or not e.adabn     # the running statistics are a calibration
        self._b, self._a = b, a
        self._prepared = False
        self.lib = _lib.load()
        self.device = e.device
        self.dtype = dtype
        self.vote = int(vote)
        self.phase = int(phase)
        self.max_windows = int(max_windows_per_push)
        cfg = self._cfg = _config(dtype, self.max_windows, self.vote, self.phase, b, a)
        self.mean_std = torch.stack([_channels(mean, self.device), _channels(std, self.device)]).contiguous()
        nbytes = (self.lib.cp_online_workspace_bytes if adapt is None else self.lib.cp_online_adapt_workspace_bytes)(self.max_windows, cfg.dtype)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.n_seen = 0
        self.class_ids: Optional[torch.Tensor] = None
        self._enroll_rec = {}
        self._map = None                                   # electrode map: (src, fill) numpy, and its device copy
        self._map_dev = None
        self._user_projection = None                       # a user's (W, b) f32 on the device: set_projection / finetune
        self.refresh()
        if classes is not None:
            self.set_classes(classes)

    # ------------------------------------------------------------------ helpers
    def _ws(self):
        return self.ws.data_ptr(), self.ws.numel()

    def tail_view(self) -> torch.Tensor:
        """(max_windows_per_push, 512) in the compute dtype: the tail inputs (fc7's output) the last push left in the
        workspace, as a view of the workspace tensor (cp_online_tail_offset; no copy, no launch).  Row r belongs to window r
        of the last chain of launches (a push of more than max_windows_per_push windows runs several) and stays valid until
        the next call that runs the encoder on this workspace."""
        return _tail_view(self, 1, 0, self.max_windows, self.adapt is not None, False)

    # ------------------------------------------------------------------ API
    def refresh(self):
        """Fold the model's current weights and running statistics into the decoder (after an optimiser step or a
        load_state_dict; until then the decoder keeps the copy of the last fold).  A class table that comes from the model
        (one-hot ids, glove rows) is derived again too, which empties the vote ring.  The adaptive form re-reads weights, gamma
        and beta and keeps its BatchNorm statistics.  A user's projection (`set_projection`, `finetune`) is kept: it is
        installed again over the model's."""
        e = self.engine
        if self.adapt is None:
            _lib.check(self.lib.cp_online_prepare(C.byref(self._cfg), C.byref(e._p), C.byref(e._bn), C.c_float(1e-5), *self._ws(),
                                                  self._stream()), "cp_online_prepare")
        else:
            bn = C.byref(e._bn) if not (e.adabn or self._prepared) else None
            _lib.check(self.lib.cp_online_adapt_prepare(C.byref(self._cfg), C.byref(e._p), bn, C.c_float(1e-5), C.c_double(self.adapt),
                                                        *self._ws(), self._stream()), "cp_online_adapt_prepare")
        self._prepared = True
        if self._user_projection is not None:              # the user's head survives, as an enrolled table does
            self._install_projection()
        if self.class_ids is not None and self._source[2] is None:
            classes, glove, _, ids = self._source
            self.set_classes(classes, glove=glove, ids=ids)

    def set_classes(self, classes=None, *, glove=None, table=None, ids=None):
        """The grasps to choose from, one of:
        classes: class ids of the model's one-hot table (row k = W_easy[:, id] + b_easy);
        glove: (K, 20) glove rows through the model's glove encoder in eval mode (zero-shot grasps), ids default 0..K-1;
        table: (K, 16) class embeddings, ids default 0..K-1.
        Rows are L2-normalised once, here.  Outputs report ids; ties go to the smallest id.  Empties the vote ring and keeps the
        filter state."""
        tab, ids_t = _class_table(self.engine, classes, glove, table, ids)
        self._source = (classes, glove, table, ids)
        self._table = tab
        self._enroll_rec.clear()                               # the accumulator is laid out by the id list
        self.class_ids = ids_t.to(torch.int32)
        self._ids_dev = self.class_ids.to(self.device)
        _lib.check(self.lib.cp_online_set_classes(C.byref(self._cfg), *self._ws(), self._table.data_ptr(), self._ids_dev.data_ptr(),
                                                  int(ids_t.numel()), self._stream()), "cp_online_set_classes")

    def reset(self):
        """Start a new stream: filter, RMS history, sample count and vote ring to zero; classes and weights (and the adaptive
        form's BatchNorm statistics: the same user keeps their calibration) stay."""
        _lib.check(self.lib.cp_online_reset(C.byref(self._cfg), *self._ws(), self._stream()), "cp_online_reset")
        self.n_seen = 0

    def set_channel_map(self, src=None, fill=None):
        """Which physical electrode feeds each model channel.  src: 12 integers, src[d] the raw column 0..11 that model channel d
        reads, or -1: masked; it need not be a permutation (a dead electrode may be replaced by a neighbour).  fill: what a
        masked channel emits in normalised units, one value or 12 (default 0.0, the training mean); read only where src is -1.
        src=None clears the map; the identity map decodes as no map does.

        With a map model channel d filters raw column src[d] with its own filter state, normalises with mean[d] and std[d] and
        fills column d of the windows, so a mapped decoder fed `raw` equals an unmapped one fed `raw[:, src]` bit for bit, and
        everything behind the front end -- the encoder, a `CommandGate`, a `GraspDrive` and its `bad` electrodes, `enroll`,
        `calibrate` -- sees model channels.  A masked channel emits `fill` exactly; its filter keeps running on zeros.
        Changing the map in mid-stream leaves a filter transient on the changed channels, as plugging a cable would;
        `reset()` clears it.  The map survives `reset()`, `refresh()` and `set_classes()`."""
        m = _check_map(src, fill)
        self._map = m
        self._map_dev = None if m is None else _map_on_device(m, self.device)

    def channel_map(self):
        """None, or (src (12,) int32, fill (12,) float32) numpy arrays as `set_channel_map` took them."""
        return None if self._map is None else (self._map[0].copy(), self._map[1].copy())

    def _map_of(self, key):
        return self._map

    def push(self, raw: torch.Tensor, return_logits: bool = False, return_windows: bool = False, return_embeddings: bool = False):
        """raw (n, 12) f32 on the GPU: the next n samples of the stream.  Returns (pred, voted[, logits][, windows][, embeddings])
        for the M = windows_emitted(n_seen, n, phase) windows the chunk completes: pred, voted (M,) int32 class ids, logits
        (M, K) f32, windows (M, 12) f32 (the normalised windows, a test aid), embeddings (M, 16) f32 (z / |z| of every window:
        what the tail multiplies with the class rows, and what a `track.PrototypeTracker` reads)."""
        if self.class_ids is None:
            raise _lib.CpNativeError("set_classes() first")
        if not self.calibrated:
            raise _lib.CpNativeError("an AdaBN model has no BatchNorm statistics: calibrate() first")
        _check_raw(raw)
        raw = raw.contiguous()
        K = self.class_ids.numel()
        step = STRIDE * self.max_windows
        outs = []
        for s in range(0, max(raw.shape[0], 1), step):
            piece = raw[s:s + step]
            n = piece.shape[0]
            if n == 0:
                break
            M = windows_emitted(self.n_seen, n, self.phase)
            pv = torch.empty(2, max(M, 1), dtype=torch.int32, device=self.device)     # (an empty tensor's pointer is NULL)
            pred, voted = pv[0, :M], pv[1, :M]
            logits = torch.empty(M, K, dtype=torch.float32, device=self.device) if return_logits else None
            wins = torch.empty(M, EMG_DIM, dtype=torch.float32, device=self.device) if return_windows else None
            emb = torch.empty(M, CP_D_E, dtype=torch.float32, device=self.device) if return_embeddings else None
            name = "cp_online_push" if self.adapt is None else "cp_online_adapt_push"
            cmap = () if self._map_dev is None else (self._map_dev[0].data_ptr(), self._map_dev[1].data_ptr())
            if return_embeddings:                              # the mapped entry with one more destination; no map: NULL, NULL
                fn, cmap, tail = getattr(self.lib, name + "_embed"), cmap or (None, None), (emb.data_ptr(),)
            else:
                fn, tail = getattr(self.lib, name + "_mapped" if cmap else name), ()
            _lib.check(fn(C.byref(self._cfg), *self._ws(), piece.data_ptr(), n, self.mean_std.data_ptr(), *cmap,
                          pv[0].data_ptr(), pv[1].data_ptr(), logits.data_ptr() if logits is not None else None,
                          wins.data_ptr() if wins is not None else None, *tail, self._stream()), name)
            self.n_seen += n
            outs.append((pred, voted, logits, wins, emb))
        if not outs:
            outs.append((torch.empty(0, dtype=torch.int32, device=self.device),) * 2
                        + (torch.empty(0, K, device=self.device), torch.empty(0, EMG_DIM, device=self.device),
                           torch.empty(0, CP_D_E, device=self.device)))

        def cat(i):
            parts = [o[i] for o in outs]
            return parts[0] if len(parts) == 1 else torch.cat(parts)

        res = [cat(0), cat(1)]
        if return_logits:
            res.append(cat(2))
        if return_windows:
            res.append(cat(3))
        if return_embeddings:
            res.append(cat(4))
        return tuple(res)

    # ------------------------------------------------------------------ class enrolment
    def enroll(self, raw: torch.Tensor, labels, *, mix: float = 1.0, min_windows: int = 25, add: bool = False,
               accumulate: bool = False) -> dict:
        """Class rows from the user's own signals (cosine prototypes, no gradient).  raw (n, 12) f32 on the GPU: a cued
        recording of the user, a stream of its own (the live filter state, sample count and vote ring are not touched);
        labels (n,) integers: the class id each raw sample was cued with, negative for "not labelled" (`window_labels` gives
        the rule).  Every labelled window's z / |z| -- computed as a push computes it; the adaptive form with its current
        statistics frozen, whatever alpha is -- is added to a float64 accumulator per class, in window order.  Then each class
        with at least `min_windows` windows gets the row (1 - mix) E_c + mix S_c / |S_c| (E_c: its current unit row, S_c: its
        sum); the others keep their row.  mix = 0 reproduces the current table exactly.  The new table goes in as
        `set_classes(table=...)` does: the vote ring empties and `refresh()` no longer derives the table from the model.

        add: a label that is not in `class_ids` is a ValueError, or with add=True a new class whose row is its prototype
        alone (it needs min_windows windows; at most 64 classes in all).  accumulate=True only adds to the accumulator and
        leaves the table alone, so several recordings can be enrolled before the table changes; the accumulator lives until
        `enroll_reset()` or the next `set_classes()`.  Returns {class id: windows accumulated so far}.

        Prototypes belong to the weights and statistics they were taken with: enrol after `calibrate()`, and again (after
        `enroll_reset()`) after a `refresh()` that changed the weights.  Under an electrode map (`set_channel_map`) the
        recording is read through the map, so the prototypes are taken in model channels."""
        return self._enroll(None, raw, labels, mix, min_windows, add, accumulate)

    def enroll_reset(self):
        """Forget the windows accumulated so far (the class table stays)."""
        self._enroll_rec.clear()

    def class_table(self):
        """(rows (K, 16) f32 on the GPU, ids (K,) int32): the class table as `set_classes(table=rows, ids=ids)` takes it, so a
        user's table can be stored and put back; the decoder normalises the rows the same way each time, and a table put
        back decodes bit for bit as this one does."""
        if self.class_ids is None:
            raise _lib.CpNativeError("set_classes() first")
        return self._table.clone(), self.class_ids.clone()

    def _enroll_view(self, key):
        if self.class_ids is None:
            return None, None, self.calibrated
        return self.class_ids.numpy().astype(np.int64), self._table, self.calibrated

    def _enroll_call(self, key, *args):
        fn, name = (self.lib.cp_online_enroll, "cp_online_enroll") if self.adapt is None \
            else (self.lib.cp_online_adapt_enroll, "cp_online_adapt_enroll")
        _lib.check(fn(C.byref(self._cfg), *self._ws(), *args, self._stream()), name)

    def _enroll_install(self, key, table, ids):
        self.set_classes(table=table, ids=ids)

    # ------------------------------------------------------------------ head fine-tuning
    def finetune(self, raw: torch.Tensor, labels, *, steps: int = 100, lr: float = 1e-3, lr_rows: Optional[float] = None,
                 scale: float = 1.0, anchor: float = 0.0, balanced: bool = True, train_projection: bool = True,
                 train_rows: bool = True, min_windows: int = 25, return_loss: bool = False):
        """The user's own head by gradient: the projection (16 x 512 + 16) and the class rows (K x 16) are trained with the
        loss the model was trained with on the labelled windows of a cued recording; the shared encoder is not touched.
        raw (n, 12) f32 on the GPU and labels (n,) as `enroll` takes them (a stream of its own, read through the electrode
        map); a label that is not in `class_ids` is a ValueError, as is a class with 1..min_windows-1 windows (a class
        without windows keeps its row's direction but for what the others' gradients do to it).

        The decoder's own encoder embeds the windows once (the adaptive form with its current statistics frozen:
        `bn_statistics()` does not move), then `steps` Adam steps run on the device without a host synchronisation
        (include/cpnative.h, "head fine-tuning"; `finetune.finetune_reference` is the definition): rates lr (projection) and
        lr_rows (rows; default lr); scale multiplies the cosines (1.0: the reference's loss; for a model trained with
        Model(temperature=...) pass `model.temperature()`, the tau its encoder was trained at); anchor pulls every trained
        tensor back to where it started with anchor * (theta - theta_0); balanced weighs every class with windows alike,
        else every window alike.  Training starts from `projection()` and the rows of `class_table()` and ends by installing
        what it trained: `set_projection(W, b)` (train_projection) and `set_classes(table=E, ids=...)` (train_rows), so the
        vote ring empties, `refresh()` keeps both, and `projection()` / `class_table()` return them for storage.  A tensor that
        is not trained stays bit-identical; steps=0 changes nothing at all.

        Returns {class id: labelled windows}; with return_loss=True also the loss of every step, (steps,) float64 on the GPU
        (entry 0 is the cross-entropy of the logits a push returns for these windows).  A head belongs to the weights and
        statistics it was trained with: fine-tune after `calibrate()`, and again after a `refresh()` that changed the model."""
        return self._finetune(None, raw, labels, steps, lr, lr_rows, scale, anchor, balanced, bool(train_projection), bool(train_rows),
                              min_windows, return_loss)

    def _entry(self, name: str):
        """the C entry cp_online_<name> of this decoder's form"""
        full = ("cp_online_" if self.adapt is None else "cp_online_adapt_") + name
        return getattr(self.lib, full), full

    def _tail_inputs_call(self, key, *args):
        fn, name = self._entry("tail_inputs")
        _lib.check(fn(C.byref(self._cfg), *self._ws(), *args, self._stream()), name)

    def _projection_read(self, key):
        W = torch.empty(CP_D_E, 512, dtype=torch.float32, device=self.device)
        b = torch.empty(CP_D_E, dtype=torch.float32, device=self.device)
        fn, name = self._entry("projection")
        _lib.check(fn(C.byref(self._cfg), *self._ws(), W.data_ptr(), b.data_ptr(), self._stream()), name)
        return W, b

    def _finetune_install(self, key, W, b, E, ids):
        if W is not None:
            self.set_projection(W, b)
        if E is not None:
            self.set_classes(table=E, ids=ids)

    def projection(self):
        """(W (16, 512) f32, b (16,) f32) on the GPU: the projection the tail multiplies by, widened from the compute dtype,
        and its bias -- the model's (BatchNorm 9 folded in; the adaptive form: a zero bias) or the user's.  As
        `set_projection(W, b)` takes them: a projection stored and put back decodes bit for bit as this one does."""
        return self._projection_read(None)

    def set_projection(self, W, b):
        """Install a user's projection: W (16, 512) and b (16,) f32 (rounded to the compute dtype once, here).  `refresh()`
        keeps it -- it belongs to the user, not to the model -- until `reset_projection()`.  Stream state, vote ring and
        classes stay."""
        W = torch.as_tensor(W, dtype=torch.float32).to(self.device).contiguous()
        b = torch.as_tensor(b, dtype=torch.float32).to(self.device).contiguous()
        if tuple(W.shape) != (CP_D_E, 512) or tuple(b.shape) != (CP_D_E,):
            raise ValueError(f"W must be ({CP_D_E}, 512) and b ({CP_D_E},)")
        self._user_projection = (W.clone(), b.clone())
        self._install_projection()

    def _install_projection(self):
        W, b = self._user_projection
        fn, name = self._entry("set_projection")
        _lib.check(fn(C.byref(self._cfg), *self._ws(), W.data_ptr(), b.data_ptr(), self._stream()), name)

    def reset_projection(self):
        """Drop the user's projection: the model's is folded in again (a `refresh()` without it), and the decoder's outputs
        are the model's bit for bit."""
        self._user_projection = None
        self.refresh()

    # ------------------------------------------------------------------ adaptive form
    def _need_adapt(self, what: str):
        if self.adapt is None:
            raise _lib.CpNativeError(f"{what} needs the adaptive form: OnlineDecoder(..., adapt=alpha)")

    def calibration_windows(self, raw: torch.Tensor) -> torch.Tensor:
        """The windows a fresh stream would emit for `raw` (n, 12), by the offline path: preprocess_segments + normalize_ with
        this decoder's filter, phase, mean and std, in model channels under the decoder's electrode map."""
        return _calibration_windows(raw, self._b, self._a, self.phase, self.mean_std, self._map)

    def calibrate(self, raw: torch.Tensor):
        """AdaBN calibration from a recording raw (n, 12) f32 on the GPU: every BatchNorm's statistics become the batch
        statistics of the recording's windows, layer by layer (include/cpnative.h).  Stream state, vote ring and classes stay.
        Under an electrode map the windows, and so the statistics, are taken in model channels."""
        self._need_adapt("calibrate()")
        if raw.dim() != 2 or windows_before(raw.shape[0], self.phase) < 2:
            raise ValueError("calibration takes at least 2 windows")
        w = self.calibration_windows(raw).contiguous()
        scratch = torch.empty(self.lib.cp_online_adapt_calibrate_scratch_bytes(w.shape[0], self._cfg.dtype), dtype=torch.uint8,
                              device=self.device)
        _lib.check(self.lib.cp_online_adapt_calibrate(C.byref(self._cfg), *self._ws(), w.data_ptr(), w.shape[0], scratch.data_ptr(),
                                                      scratch.numel(), self._stream()), "cp_online_adapt_calibrate")
        self.calibrated = True

    def bn_statistics(self) -> torch.Tensor:
        """(9, 2, 512) float64 on the GPU: mean and variance of each BatchNorm as the next window sees them (conv BatchNorms
        fill channels 0..63)."""
        self._need_adapt("bn_statistics()")
        out = torch.zeros(9, 2, 512, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.cp_online_adapt_statistics(C.byref(self._cfg), *self._ws(), out.data_ptr(), self._stream()),
                   "cp_online_adapt_statistics")
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# many streams: one model, one chain of launches per push (cp_online_multi_*, csrc/online_multi.cuh)
# ---------------------------------------------------------------------------------------------------------------------------
MAX_STREAMS = _lib.CP_ONLINE_MULTI_MAX_STREAMS
DEFAULT_MAX_ROWS = 4096


def _windows_before_np(n, phase: int) -> np.ndarray:
    return np.maximum(0, (np.asarray(n, dtype=np.int64) - phase - 2 * WINDOW_EDGE - 1 + STRIDE) // STRIDE)


def packed_rows(n_seen, counts, phase: int = 0):
    """Where a multi-stream push packs each stream's windows: (row0, m), int64 arrays over streams, with m[s] =
    windows_emitted(n_seen[s], counts[s], phase) and row0 the exclusive prefix sum of m (include/cpnative.h)."""
    seen = np.asarray(n_seen, dtype=np.int64)
    m = _windows_before_np(seen + np.asarray(counts, dtype=np.int64), phase) - _windows_before_np(seen, phase)
    row0 = np.zeros_like(m)
    np.cumsum(m[:-1], out=row0[1:])
    return row0, m


def plan_push(n_seen, counts, phase: int, max_windows: int, max_rows: int):
    """Split a push of counts[s] samples per stream into rounds that each emit at most `max_windows` windows per stream and
    `max_rows` windows in all: a list of int64 arrays (samples per stream), whose sum per stream is counts[s].  Every stream's
    samples keep their order; a stream's outputs do not depend on how its samples are chunked."""
    seen = np.array(n_seen, dtype=np.int64)
    left = np.array(counts, dtype=np.int64)
    rounds = []
    while left.any():
        take = np.minimum(left, STRIDE * max_windows)                  # 20 W samples complete at most W windows
        _, m = packed_rows(seen, take, phase)
        if m.sum() > max_rows:
            rows = 0
            for s in np.nonzero(take)[0]:
                k = max_rows - rows
                if m[s] > k:                                            # the most samples that complete k windows
                    first = int(_windows_before_np(seen[s], phase))
                    take[s] = min(take[s], STRIDE * (first + k + 1) + phase - 2 * WINDOW_EDGE - seen[s])
                    m[s] = windows_emitted(int(seen[s]), int(take[s]), phase)
                rows += int(m[s])
        rounds.append(take)
        seen += take
        left -= take
    return rounds


class _MultiStreamBase(_EnrollMixin):
    """What the multi-stream decoders share: settings, workspace, per-stream class tables and sample counts, packing and
    splitting of pushes.  Subclasses name their C entries (_ENTRY: cp_online_multi or cp_online_multi_adapt) and prepare."""
    _WHO = "MultiStreamDecoder"
    _ENTRY = "cp_online_multi"

    def _setup(self, e: Engine, mean, std, n_streams, vote, dtype, phase, max_windows_per_push, max_rows, b, a,
               stream_projections: bool = False):
        dtype = _check_settings(e, dtype, vote, phase, max_windows_per_push, self._WHO)
        if not 1 <= int(n_streams) <= MAX_STREAMS:
            raise ValueError(f"n_streams must lie in 1..{MAX_STREAMS}")
        if max_rows is None:
            max_rows = max(int(max_windows_per_push), min(int(n_streams) * int(max_windows_per_push), DEFAULT_MAX_ROWS))
        if not 1 <= int(max_rows) <= _lib.CP_ONLINE_MULTI_MAX_ROWS:
            raise ValueError(f"max_rows must lie in 1..{_lib.CP_ONLINE_MULTI_MAX_ROWS}")
        b, a = _filter(b, a)
        self.engine = e
        self.lib = _lib.load()
        self.device = e.device
        self.dtype = dtype
        self.vote = int(vote)
        self.phase = int(phase)
        self.max_windows = int(max_windows_per_push)
        self.max_rows = int(max_rows)
        self.n_streams = int(n_streams)
        self._b, self._a = b, a
        self._cfg = _config(dtype, self.max_windows, self.vote, self.phase, b, a)
        self.mean_std = torch.stack([_channels(mean, self.device), _channels(std, self.device)]).contiguous()
        nbytes = getattr(self.lib, self._ENTRY + "_workspace_bytes")(self.n_streams, self.max_rows, self._cfg.dtype)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._seen = np.zeros(self.n_streams, dtype=np.int64)
        self.class_ids = [None] * self.n_streams           # per stream: sorted ids (K,) int32, or None before set_classes
        self._source = [None] * self.n_streams
        self._tables = [None] * self.n_streams             # kept alive until the next set_classes of the stream
        self._has_table = np.zeros(self.n_streams, dtype=bool)
        self._k = [0] * self.n_streams                     # classes per stream
        self._counts_cache = None
        self._enroll_rec = {}
        self._maps = [None] * self.n_streams               # electrode maps: (src, fill) numpy per stream, None: the identity
        self._map_src = torch.arange(EMG_DIM, dtype=torch.int32, device=self.device).repeat(self.n_streams, 1).contiguous()
        self._map_fill = torch.zeros(self.n_streams, EMG_DIM, dtype=torch.float32, device=self.device)
        self.stream_projections = bool(stream_projections)
        self._bank = None                                  # the streams' own projections (cp_online_projections_*): zeros, none set
        if self.stream_projections:
            self._shared_projection = False                # (this decoder's: the class attribute stays)
            self._bank = torch.zeros(self.lib.cp_online_projections_bytes(self.n_streams, self._cfg.dtype), dtype=torch.uint8,
                                     device=self.device)
            self._own_projection = np.zeros(self.n_streams, dtype=bool)

    # ------------------------------------------------------------------ helpers
    def _args(self):
        return (C.byref(self._cfg), self.n_streams, self.max_rows, self.ws.data_ptr(), self.ws.numel())

    def tail_view(self) -> torch.Tensor:
        """(max_rows, 512) in the compute dtype: the tail inputs (fc7's output) the last push left in the workspace, as a view
        of the workspace tensor (cp_online_tail_offset; no copy, no launch).  Row r belongs to packed row r (stream, window)
        of the last chain of launches and stays valid until the next call that runs the encoder on this workspace."""
        return _tail_view(self, self.n_streams, self.max_rows, self.max_rows, self._ENTRY.endswith("adapt"), True)

    def _bank_args(self):
        return (self._bank.data_ptr(), self._bank.numel())

    def _slot_args(self, s: int):
        """what the cp_online_projections_* entries take in front: dtype, bank, bank_bytes, n_streams, index"""
        return (self._cfg.dtype, *self._bank_args(), self.n_streams, s)

    def _index(self, stream) -> int:
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {stream!r}")
        return int(stream)

    @property
    def n_seen(self) -> np.ndarray:
        """samples pushed into each stream since its last reset"""
        return self._seen.copy()

    # ------------------------------------------------------------------ API
    def _set_model_tables(self):
        """derive the class tables that come from the model again"""
        for s, src in enumerate(self._source):
            if src is not None and src[2] is None:
                classes, glove, _, ids = src
                self.set_classes(s, classes, glove=glove, ids=ids)

    def set_classes(self, stream: int, classes=None, *, glove=None, table=None, ids=None):
        """The class table of one stream, as OnlineDecoder.set_classes: classes= (one-hot ids), glove= (K, 20) or table= (K, 16),
        ids.  Empties that stream's vote ring; its filter state and every other stream stay."""
        s = self._index(stream)
        tab, ids_t = _class_table(self.engine, classes, glove, table, ids)
        ids32 = ids_t.to(torch.int32)
        ids_dev = ids32.to(self.device)
        _lib.check(self.lib.cp_online_multi_set_classes(*self._args(), s, tab.data_ptr(), ids_dev.data_ptr(), int(ids32.numel()),
                                                        self._stream()), "cp_online_multi_set_classes")
        self._source[s] = (classes, glove, table, ids)
        self._tables[s] = (tab, ids_dev)
        self.class_ids[s] = ids32
        self._has_table[s] = True
        self._k[s] = int(ids32.numel())
        self._enroll_rec.pop(s, None)                          # the accumulator is laid out by the id list

    def set_channel_map(self, stream: int, src=None, fill=None):
        """The electrode map of one stream, as `OnlineDecoder.set_channel_map`: src[d] the raw column that feeds model channel
        d or -1 (masked, emits fill[d]); src=None clears it.  The maps of all streams live in one small device array that a
        push reads in its front-end launch; the other streams, and this stream's state, are not touched.  The map survives
        `reset()`, `refresh()` and `set_classes()`; under it `enroll` and `calibrate` of the stream work in model channels."""
        s = self._index(stream)
        m = _check_map(src, fill)
        self._maps[s] = m
        ident = (np.arange(EMG_DIM, dtype=np.int32), np.zeros(EMG_DIM, dtype=np.float32))
        src_dev, fill_dev = _map_on_device(m if m is not None else ident, self.device)
        self._map_src[s].copy_(src_dev)
        self._map_fill[s].copy_(fill_dev)

    def channel_map(self, stream: int):
        """None, or (src (12,) int32, fill (12,) float32) numpy arrays of one stream."""
        m = self._maps[self._index(stream)]
        return None if m is None else (m[0].copy(), m[1].copy())

    def _map_of(self, s):
        return self._maps[s]

    def enroll(self, stream: int, raw: torch.Tensor, labels, *, mix: float = 1.0, min_windows: int = 25, add: bool = False,
               accumulate: bool = False) -> dict:
        """`OnlineDecoder.enroll` for one stream: its class table becomes, bit for bit, the one its own `OnlineDecoder` gets
        from the same call; no other stream's table, state or statistics change."""
        return self._enroll(self._index(stream), raw, labels, mix, min_windows, add, accumulate)

    def enroll_reset(self, stream: int):
        """Forget the windows accumulated for one stream (its class table stays)."""
        self._enroll_rec.pop(self._index(stream), None)

    def class_table(self, stream: int):
        """(rows (K, 16) f32 on the GPU, ids (K,) int32) of one stream, as `OnlineDecoder.class_table`."""
        s = self._index(stream)
        if not self._has_table[s]:
            raise _lib.CpNativeError(f"stream {s} has no class table: set_classes({s}, ...) first")
        return self._tables[s][0].clone(), self.class_ids[s].clone()

    def _enroll_calibrated(self, s: int) -> bool:
        return True

    def _enroll_view(self, s):
        if not self._has_table[s]:
            return None, None, self._enroll_calibrated(s)
        return self.class_ids[s].numpy().astype(np.int64), self._tables[s][0], self._enroll_calibrated(s)

    def _enroll_call(self, s, *args):
        if self._bank is not None:                             # with the projection stream s decodes with
            name = self._ENTRY + "_enroll_proj"
            _lib.check(getattr(self.lib, name)(*self._args(), s, *self._bank_args(), *args, self._stream()), name)
            return
        self._enroll_call_shared(s, *args)

    def _enroll_call_shared(self, s, *args):
        _lib.check(self.lib.cp_online_multi_enroll(*self._args(), *args, self._stream()), "cp_online_multi_enroll")

    def _enroll_install(self, s, table, ids):
        self.set_classes(s, table=table, ids=ids)

    _shared_projection = True

    def finetune(self, stream: int, raw: torch.Tensor, labels, *, steps: int = 100, lr: float = 1e-3, lr_rows: Optional[float] = None,
                 scale: float = 1.0, anchor: float = 0.0, balanced: bool = True, train_projection: bool = False,
                 train_rows: bool = True, min_windows: int = 25, return_loss: bool = False):
        """`OnlineDecoder.finetune` for one stream's class rows: its class table becomes, bit for bit, the one its own
        `OnlineDecoder.finetune(train_projection=False)` gets from the same call; no other stream's table, state or statistics
        change.  Without `stream_projections=True` the projection is shared by all streams, so train_projection=True is a
        ValueError.  With it the stream's own head is trained as `OnlineDecoder.finetune` trains one: from `projection(stream)`
        and the stream's rows, into the stream's slot (`set_projection(stream, W, b)`) and its class table, bit for bit what
        the stream's own `OnlineDecoder` gets; nothing of any other stream changes."""
        return self._finetune(self._index(stream), raw, labels, steps, lr, lr_rows, scale, anchor, balanced, bool(train_projection),
                              bool(train_rows), min_windows, return_loss)

    def _tail_inputs_call(self, s, *args):
        _lib.check(self.lib.cp_online_multi_tail_inputs(*self._args(), *args, self._stream()), "cp_online_multi_tail_inputs")

    def _projection_read(self, s):
        W = torch.empty(CP_D_E, 512, dtype=torch.float32, device=self.device)
        b = torch.empty(CP_D_E, dtype=torch.float32, device=self.device)
        if self._bank is not None and self._own_projection[s]:
            _lib.check(self.lib.cp_online_projections_get(*self._slot_args(s), W.data_ptr(), b.data_ptr(), None, self._stream()),
                       "cp_online_projections_get")
            return W, b
        name = self._ENTRY + "_projection"
        _lib.check(getattr(self.lib, name)(*self._args(), W.data_ptr(), b.data_ptr(), self._stream()), name)
        return W, b

    def _finetune_install(self, s, W, b, E, ids):
        if W is not None:                                      # (train_projection: only with stream_projections=True)
            self.set_projection(s, W, b)
        if E is not None:
            self.set_classes(s, table=E, ids=ids)

    # ------------------------------------------------------------------ per-stream projections (stream_projections=True)
    def _need_bank(self, what: str):
        if self._bank is None:
            raise _lib.CpNativeError(f"{what}: the streams of this decoder share one projection; build it with "
                                     "stream_projections=True to give each stream a slot of its own")

    def set_projection(self, stream: int, W, b):
        """Install a user's projection for one stream, as `OnlineDecoder.set_projection`: W (16, 512) and b (16,) finite f32
        (rounded to the compute dtype once, here).  It lives in the stream's slot of the decoder's projection bank, outside
        the workspace: `refresh()` keeps it, `reset_projection(stream)` drops it, and from the next push on the stream's
        outputs equal bit for bit those of its own `OnlineDecoder` with the same projection set.  The stream's state, vote ring
        and classes, and everything of the other streams, stay.  Needs `stream_projections=True`."""
        self._need_bank("set_projection")
        s = self._index(stream)
        W, b = _check_projection(W, b)
        W, b = W.to(self.device).contiguous(), b.to(self.device).contiguous()
        _lib.check(self.lib.cp_online_projections_set(*self._slot_args(s), W.data_ptr(), b.data_ptr(), self._stream()),
                   "cp_online_projections_set")
        self._own_projection[s] = True

    def projection(self, stream: int):
        """(W (16, 512) f32, b (16,) f32) on the GPU: the projection the tail multiplies stream `stream`'s rows by -- its own
        if one is set, else the one all streams share --, widened from the compute dtype, as `OnlineDecoder.projection`."""
        return self._projection_read(self._index(stream))

    def has_projection(self, stream: int) -> bool:
        """whether the stream decodes with a projection of its own (always False without `stream_projections=True`)"""
        s = self._index(stream)
        return bool(self._bank is not None and self._own_projection[s])

    def reset_projection(self, stream=None):
        """Drop the own projection of one stream, or of all (stream=None): from the next push on they decode with the shared
        projection again, bit for bit as streams that never had one.  Needs `stream_projections=True`."""
        self._need_bank("reset_projection")
        s = -1 if stream is None else self._index(stream)
        _lib.check(self.lib.cp_online_projections_clear(*self._slot_args(s), self._stream()), "cp_online_projections_clear")
        if s < 0:
            self._own_projection[:] = False
        else:
            self._own_projection[s] = False

    def reset(self, streams=None):
        """Start new streams: filter, RMS history, sample count and vote ring of the listed streams (default: all) to zero;
        their classes, the weights and the other streams stay."""
        if streams is None:
            _lib.check(self.lib.cp_online_multi_reset(*self._args(), -1, self._stream()), "cp_online_multi_reset")
            self._seen[:] = 0
            return
        idx = sorted({self._index(s) for s in streams})
        for s in idx:
            _lib.check(self.lib.cp_online_multi_reset(*self._args(), s, self._stream()), "cp_online_multi_reset")
            self._seen[s] = 0

    def push(self, chunks, return_logits: bool = False, return_windows: bool = False, return_embeddings: bool = False):
        """chunks: n_streams entries, each None or an (n_s, 12) float32 GPU tensor, the next samples of stream s.  Returns one
        tuple per stream, (pred, voted[, logits][, windows][, embeddings]) for its windows_emitted(n_seen[s], n_s, phase)
        windows: views into the packed outputs (pred, voted int32 class ids, logits (M_s, K_s) f32, windows (M_s, 12) f32,
        embeddings (M_s, 16) f32, z / |z| of every window)."""
        if isinstance(chunks, torch.Tensor) or len(chunks) != self.n_streams:
            raise ValueError(f"chunks must be a sequence of {self.n_streams} entries (None or (n, 12) tensors)")
        counts, parts = [], []
        for c in chunks:
            if c is None:
                counts.append(0)
                continue
            _check_raw(c, "each chunk")
            counts.append(int(c.shape[0]))
            if c.shape[0]:
                parts.append(c)
        if not parts:
            raw = torch.empty(0, EMG_DIM, dtype=torch.float32, device=self.device)
        elif len(parts) == 1:
            raw = parts[0].contiguous()
        else:
            raw = torch.cat(parts)
        return self._push(raw, np.asarray(counts, dtype=np.int64), return_logits, return_windows, return_embeddings)

    def push_packed(self, raw: torch.Tensor, counts, return_logits: bool = False, return_windows: bool = False,
                    return_embeddings: bool = False):
        """As push, for samples already packed in stream order: raw (sum(counts), 12) float32 on the GPU, counts[s] >= 0 the
        samples of stream s."""
        _check_raw(raw)
        cnt = np.asarray(counts, dtype=np.int64).reshape(-1)
        if cnt.shape[0] != self.n_streams:
            raise ValueError(f"counts must hold {self.n_streams} entries")
        if (cnt < 0).any():
            raise ValueError("counts must be >= 0")
        if int(cnt.sum()) != raw.shape[0]:
            raise ValueError(f"counts sum to {int(cnt.sum())} samples, raw holds {raw.shape[0]}")
        return self._push(raw.contiguous(), cnt, return_logits, return_windows, return_embeddings)

    def _check_push(self, counts: np.ndarray):
        """refusals of a subclass, before anything is enqueued"""

    def _counts_on_device(self, take: np.ndarray) -> torch.Tensor:
        """take as int32 on the device.  A stream of pushes usually repeats its counts: the last device copy is reused (it is
        only ever read), else a fresh one goes through pinned memory, whose block torch's host allocator keeps until the copy
        has run."""
        key = (take.tobytes(), self._stream())
        if self._counts_cache is not None and self._counts_cache[0] == key:
            return self._counts_cache[1]
        dev = torch.from_numpy(take.astype(np.int32)).pin_memory().to(self.device, non_blocking=True)
        self._counts_cache = (key, dev)
        return dev

    def _push(self, raw: torch.Tensor, counts: np.ndarray, return_logits: bool, return_windows: bool, return_embeddings: bool = False):
        if ((counts > 0) & ~self._has_table).any():
            s = int(np.nonzero((counts > 0) & ~self._has_table)[0][0])
            raise _lib.CpNativeError(f"stream {s} has samples but no class table: set_classes({s}, ...) first")
        self._check_push(counts)
        row0, m = packed_rows(self._seen, counts, self.phase)
        if m.max() <= self.max_windows and m.sum() <= self.max_rows:
            rounds = [(counts, raw, m)]                        # the usual case: one chain of launches
        else:
            start = np.zeros_like(counts)                      # each stream's first sample in raw
            np.cumsum(counts[:-1], out=start[1:])
            done = np.zeros_like(counts)
            seen = self._seen.copy()
            rounds = []
            for take in plan_push(self._seen, counts, self.phase, self.max_windows, self.max_rows):
                piece = torch.cat([raw[start[s] + done[s]:start[s] + done[s] + take[s]] for s in np.nonzero(take)[0]])
                rounds.append((take, piece, packed_rows(seen, take, self.phase)[1]))
                seen += take
                done += take
        outs = []                                              # per round: per-stream (pred, voted, logits, windows) views
        for take, piece, m in rounds:
            R = int(m.sum())
            pv = torch.empty(2, max(R, 1), dtype=torch.int32, device=self.device)     # (an empty tensor's pointer is NULL)
            logits = torch.empty(R, MAX_CLASSES, dtype=torch.float32, device=self.device) if return_logits else None
            wins = torch.empty(R, EMG_DIM, dtype=torch.float32, device=self.device) if return_windows else None
            emb = torch.empty(R, CP_D_E, dtype=torch.float32, device=self.device) if return_embeddings else None
            if piece.shape[0]:
                cmap = (self._map_src.data_ptr(), self._map_fill.data_ptr()) if any(m is not None for m in self._maps) else ()
                if self._bank is not None:                     # the embed entry with the bank; no map, no embeddings: NULL
                    name, cmap = "_push_proj", cmap or (None, None)
                    tail = (emb.data_ptr() if emb is not None else None, *self._bank_args())
                elif return_embeddings:                        # the mapped entry with one more destination; no map: NULL, NULL
                    name, cmap, tail = "_push_embed", cmap or (None, None), (emb.data_ptr(),)
                else:
                    name, tail = "_push_mapped" if cmap else "_push", ()
                _lib.check(getattr(self.lib, self._ENTRY + name)(
                    *self._args(), piece.data_ptr(), self._counts_on_device(take).data_ptr(), int(piece.shape[0]), R,
                    self.mean_std.data_ptr(), *cmap, pv[0].data_ptr(), pv[1].data_ptr(),
                    logits.data_ptr() if logits is not None else None, wins.data_ptr() if wins is not None else None,
                    *tail, self._stream()), self._ENTRY + "_push")
            self._seen += take
            ml = m.tolist()
            cols = [pv[0, :R].split(ml), pv[1, :R].split(ml)]
            if return_logits:
                cols.append([x[:, :k] for x, k in zip(logits.split(ml), self._k)])
            if return_windows:
                cols.append(wins.split(ml))
            if return_embeddings:
                cols.append(emb.split(ml))
            outs.append(list(zip(*cols)))
        if len(outs) == 1:
            return outs[0]
        return [tuple(torch.cat([o[s][i] for o in outs]) for i in range(len(outs[0][s]))) for s in range(self.n_streams)]


class MultiStreamDecoder(_MultiStreamBase):
    """`OnlineDecoder` for n_streams (1..256) streams at once: one model, one set of folded weights, one dtype, vote length,
    phase, filter and normalisation for all; per stream its own filter and RMS state, sample count, vote ring and class table.
    A push is one chain of ten launches for all streams, and every stream's pred, voted, logits and windows equal bit for bit
    those of an `OnlineDecoder` with the same settings and class table fed the same chunks of that stream alone.

    max_windows_per_push bounds the windows of one stream per launch chain, max_rows (default min(n_streams *
    max_windows_per_push, 4096)) the windows of all streams; larger pushes are split on the host.  stream_projections=True
    gives every stream a slot for a projection of its own (`set_projection(stream, W, b)`, `projection`, `has_projection`,
    `reset_projection`; `finetune(stream, ..., train_projection=True)` and `Readout.install(decoder, stream=)` fill it): a
    stream with one decodes, enrols and sweeps maps bit for bit as its own `OnlineDecoder` with `set_projection(W, b)`, a
    stream without one as before, still in ten launches per push; the stages behind the decoder (`CommandGate`,
    `SequenceGate`, `GraspDrive`, `PostureRows`, `MetricRows`, `PrototypeTracker`, `embed_recording`,
    `holdout.score_enrolment`, `pick_ridge(..., stream=)`) read what a push emits and need nothing.  Stock BatchNorm only: the
    adaptive form (adapt=) and AdaBN models are refused, as is fp8 (`AdaptiveMultiStreamDecoder` is the adaptive form)."""

    def __init__(self, model_or_engine, mean, std, n_streams: int, vote: int = VOTE, dtype: Optional[str] = None, phase: int = 0,
                 max_windows_per_push: int = 256, max_rows: Optional[int] = None, b=None, a=None, adapt: Optional[float] = None,
                 stream_projections: bool = False):
        e = _engine_of(model_or_engine, "MultiStreamDecoder")
        if adapt is not None:
            raise _lib.CpNativeError("MultiStreamDecoder has no adaptive form (adapt=): decode adapting streams with "
                                     "AdaptiveMultiStreamDecoder, or one with OnlineDecoder(..., adapt=alpha)")
        if e.adabn:
            raise _lib.CpNativeError("MultiStreamDecoder needs stock BatchNorm with running statistics: an AdaBN model normalises "
                                     "with the statistics of its batch (AdaptiveMultiStreamDecoder calibrates them)")
        self._setup(e, mean, std, n_streams, vote, dtype, phase, max_windows_per_push, max_rows, b, a, stream_projections)
        self.refresh()

    def refresh(self):
        """Fold the model's current weights and running statistics again (as OnlineDecoder.refresh); the class tables that come
        from the model (classes=, glove=) are derived again, which empties those streams' vote rings."""
        e = self.engine
        _lib.check(self.lib.cp_online_multi_prepare(C.byref(self._cfg), self.n_streams, self.max_rows, C.byref(e._p), C.byref(e._bn),
                                                    C.c_float(1e-5), self.ws.data_ptr(), self.ws.numel(), self._stream()),
                   "cp_online_multi_prepare")
        self._set_model_tables()



class AdaptiveMultiStreamDecoder(_MultiStreamBase):
    """`OnlineDecoder(adapt=alpha)` for n_streams (1..256) streams at once (cp_online_multi_adapt_*,
    csrc/online_multi_adapt.cuh): one model with its BatchNorms unfolded, stored once; per stream, besides what
    `MultiStreamDecoder` keeps, float64 statistics of the 9 BatchNorms and its own alpha in [0, 1) (a float for all streams,
    or one per stream; 0 freezes).  A push is one chain of twelve launches for all streams, and every stream's pred, voted,
    logits, windows and `bn_statistics` equal bit for bit those of an `OnlineDecoder(adapt=alpha_s)` with the same settings,
    class table and calibration fed the same chunks of that stream alone.  stream_projections=True as on `MultiStreamDecoder`:
    a slot per stream for a projection of its own, the twelve launches unchanged.

    Stock models start every stream at the running statistics; under an AdaBN model every stream starts uncalibrated and
    takes samples only after `calibrate(stream, raw)`.  fp8, and glove class rows under an AdaBN model, are refused."""
    _WHO = "AdaptiveMultiStreamDecoder"
    _ENTRY = "cp_online_multi_adapt"

    def __init__(self, model_or_engine, mean, std, n_streams: int, alpha, vote: int = VOTE, dtype: Optional[str] = None,
                 phase: int = 0, max_windows_per_push: int = 256, max_rows: Optional[int] = None, b=None, a=None,
                 stream_projections: bool = False):
        e = _engine_of(model_or_engine, "AdaptiveMultiStreamDecoder")
        if not 1 <= int(n_streams) <= MAX_STREAMS:
            raise ValueError(f"n_streams must lie in 1..{MAX_STREAMS}")
        alphas = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (int(n_streams),)).copy() \
            if np.ndim(alpha) == 0 else np.asarray(alpha, dtype=np.float64).reshape(-1)
        if alphas.shape[0] != int(n_streams):
            raise ValueError(f"alpha: one value, or one per stream ({int(n_streams)})")
        for x in alphas:
            self._check_alpha(x)
        self._setup(e, mean, std, n_streams, vote, dtype, phase, max_windows_per_push, max_rows, b, a, stream_projections)
        self.alpha = alphas
        self.calibrated = np.full(self.n_streams, not e.adabn)     # the running statistics are a calibration
        self._prepared = False
        self.refresh()

    @staticmethod
    def _check_alpha(x):
        if not 0.0 <= float(x) < 1.0:
            raise ValueError("alpha must lie in [0, 1)")

    def _check_push(self, counts: np.ndarray):
        bad = np.nonzero((counts > 0) & ~self.calibrated)[0]
        if bad.size:
            s = int(bad[0])
            raise _lib.CpNativeError(f"stream {s} is uncalibrated (an AdaBN model has no BatchNorm statistics): "
                                     f"calibrate({s}, raw) first")

    def _enroll_calibrated(self, s: int) -> bool:
        return bool(self.calibrated[s])

    def _enroll_call_shared(self, s, *args):
        _lib.check(self.lib.cp_online_multi_adapt_enroll(*self._args(), s, *args, self._stream()), "cp_online_multi_adapt_enroll")

    def _tail_inputs_call(self, s, *args):
        _lib.check(self.lib.cp_online_multi_adapt_tail_inputs(*self._args(), s, *args, self._stream()),
                   "cp_online_multi_adapt_tail_inputs")

    # ------------------------------------------------------------------ API
    def refresh(self):
        """Re-read the model's weights, gamma and beta; every stream keeps its BatchNorm statistics and alpha (as
        OnlineDecoder(adapt=).refresh).  Class tables that come from the model are derived again."""
        e = self.engine
        first = not self._prepared                         # the first prepare also sets the statistics (stock) and every alpha
        bn = C.byref(e._bn) if first and not e.adabn else None
        alpha = (C.c_double * self.n_streams)(*self.alpha.tolist()) if first else None
        _lib.check(self.lib.cp_online_multi_adapt_prepare(C.byref(self._cfg), self.n_streams, self.max_rows, C.byref(e._p), bn,
                                                          C.c_float(1e-5), alpha, self.ws.data_ptr(), self.ws.numel(),
                                                          self._stream()), "cp_online_multi_adapt_prepare")
        self._prepared = True
        self._set_model_tables()

    def set_alpha(self, stream: int, alpha: float):
        """The tracking rate of one stream from its next window on (0 freezes its statistics)."""
        s = self._index(stream)
        self._check_alpha(alpha)
        _lib.check(self.lib.cp_online_multi_adapt_set_alpha(*self._args(), s, C.c_double(float(alpha)), self._stream()),
                   "cp_online_multi_adapt_set_alpha")
        self.alpha[s] = float(alpha)

    def calibrate(self, stream: int, raw: torch.Tensor):
        """AdaBN calibration of one stream from a recording raw (n, 12) f32 on the GPU, as OnlineDecoder.calibrate (in model
        channels under the stream's electrode map).  No other stream's statistics, and no stream's filter state, vote ring or
        class table, change."""
        s = self._index(stream)
        if raw.dim() != 2 or windows_before(raw.shape[0], self.phase) < 2:
            raise ValueError("calibration takes at least 2 windows")
        w = _calibration_windows(raw, self._b, self._a, self.phase, self.mean_std, self._maps[s]).contiguous()
        scratch = torch.empty(self.lib.cp_online_adapt_calibrate_scratch_bytes(w.shape[0], self._cfg.dtype), dtype=torch.uint8,
                              device=self.device)
        _lib.check(self.lib.cp_online_multi_adapt_calibrate(*self._args(), s, w.data_ptr(), w.shape[0], scratch.data_ptr(),
                                                            scratch.numel(), self._stream()), "cp_online_multi_adapt_calibrate")
        self.calibrated[s] = True

    def reset_statistics(self, stream: int):
        """Hand a stream to a new user: its statistics return to the model's current running statistics (stock BatchNorm) or
        to uncalibrated (AdaBN).  With reset(stream) too, the stream is a freshly built OnlineDecoder(adapt=alpha)."""
        s = self._index(stream)
        e = self.engine
        bn = None if e.adabn else C.byref(e._bn)
        _lib.check(self.lib.cp_online_multi_adapt_reset_statistics(*self._args(), s, bn, self._stream()),
                   "cp_online_multi_adapt_reset_statistics")
        self.calibrated[s] = not e.adabn

    def bn_statistics(self, stream: int) -> torch.Tensor:
        """(9, 2, 512) float64 on the GPU: one stream's BatchNorm statistics as its next window sees them (as
        OnlineDecoder.bn_statistics)."""
        s = self._index(stream)
        out = torch.zeros(9, 2, 512, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.cp_online_multi_adapt_statistics(*self._args(), s, out.data_ptr(), self._stream()),
                   "cp_online_multi_adapt_statistics")
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# grasp command gate: rejection, weighted vote and dwell behind any of the decoders (cp_online_gate_*, csrc/online_gate.cuh)
# ---------------------------------------------------------------------------------------------------------------------------
def thresholds_from_logits(logits, labels, ids, keep: float = 0.95) -> dict:
    """Per-class cosine thresholds from a cued recording: logits (M, K) as `push(..., return_logits=True)` gives them, labels
    (M,) the label of each window (`window_labels`; negative: not labelled), ids (K,) the ascending class ids of the columns.
    For class c the windows count whose label is c and whose argmax (first maximum) is c; with v their top cosines in ascending
    order and n their number, the threshold is v[floor((1 - keep) * n)]: about the fraction `keep` of the user's own correct
    windows passes it.  Classes without such a window are left out.  {class id: threshold}; host only (numpy)."""
    lg = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    cid = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    cid = cid.reshape(-1)
    if lg.ndim != 2 or lg.shape[1] != cid.shape[0] or lg.shape[1] < 1:
        raise ValueError("logits must be (M, K) with one column per id")
    if lab.shape != (lg.shape[0],):
        raise ValueError(f"labels must hold one entry per window ({lg.shape[0]})")
    if not 0.0 < float(keep) <= 1.0:
        raise ValueError("keep must lie in (0, 1]")
    lg = lg.astype(np.float32)
    top = lg.argmax(axis=1) if lg.shape[0] else np.zeros(0, dtype=np.int64)
    out = {}
    for k, c in enumerate(cid.tolist()):
        v = np.sort(lg[(lab == c) & (top == k), k])
        if v.size:
            out[int(c)] = float(v[int(np.floor((1.0 - float(keep)) * v.size))])
    return out


def _packed_rows(views, row0, trusted: bool, width: int):
    """the rows of one launch as (tensor whose data_ptr is row 0, leading dimension): the (M_s, <= width) views as they lie if
    they are the packed output of a push (one buffer, stream order, one row stride), else a packed (rows, width) copy.
    Every view is checked; of a push's own output (trusted) only the first and the last one, which tell its one packed
    buffer from the per-stream concatenations of a push that had to be split."""
    live = [(s, v) for s, v in enumerate(views) if v is not None]
    s0, v0 = live[0]
    ld = int(v0.stride(0)) if v0.shape[0] > 1 or len(live) > 1 else max(int(v0.shape[1]), 1)
    ok = ld >= 1
    for s, v in ((live[0], live[-1]) if trusted else live):
        ok = ok and v.stride(1) == 1 and (v.shape[0] == 1 or v.stride(0) == ld) and ld >= v.shape[1] \
            and v.untyped_storage().data_ptr() == v0.untyped_storage().data_ptr() \
            and v.data_ptr() == v0.data_ptr() + v0.element_size() * ld * int(row0[s] - row0[s0])
    if ok:
        return v0, ld
    buf = torch.zeros(int(sum(v.shape[0] for _, v in live)), width, dtype=v0.dtype, device=v0.device)
    for s, v in live:
        buf[int(row0[s]):int(row0[s]) + v.shape[0], :v.shape[1]] = v
    return buf, width


def _rows_on_device(cache: dict, row0: np.ndarray, m: np.ndarray, stream: int, device) -> torch.Tensor:
    """(row0, m) of one launch as a (2, n_streams) int32 device tensor.  A stream of pushes usually repeats its row counts:
    device copies are kept (they are only ever read), a fresh one goes through pinned memory."""
    key = (row0.tobytes(), m.tobytes(), stream)
    rm = cache.get(key)
    if rm is None:
        if len(cache) >= 16:
            cache.clear()
        rm = torch.from_numpy(np.stack([row0, m]).astype(np.int32)).pin_memory().to(device, non_blocking=True)
        cache[key] = rm
    return rm


_GATE_WEIGHTS = {"count": 0, "margin": 1}
_GATE_KEYS = ("min_cosine", "default", "min_margin", "min_votes", "dwell", "release", "weight", "vote")


def _gate_settings(new: dict):
    """min_margin, min_votes, dwell, release, weight of a gate as the C config takes them, or ValueError"""
    if not isinstance(new["weight"], str) or new["weight"] not in _GATE_WEIGHTS:
        raise ValueError("weight must be 'count' or 'margin'")
    mm = float(new["min_margin"])
    if not (mm >= 0.0 and np.isfinite(mm)):
        raise ValueError("min_margin must be finite and >= 0")
    for k, low in (("min_votes", 1), ("dwell", 1), ("release", 0)):
        v = new[k]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not low <= int(v) < 2 ** 31:
            raise ValueError(f"{k} must be an int >= {low}")
    return mm, int(new["min_votes"]), int(new["dwell"]), int(new["release"]), _GATE_WEIGHTS[new["weight"]]


class CommandGate(_OnStream):
    """A command a hand can follow, from any of the four decoders: per stream one state machine on the device that reads the
    logits of every push (include/cpnative.h, cp_online_gate_*; one launch more per push, nothing is copied to the host).

    A window is accepted if its top cosine reaches `min_cosine` of its class and leads the runner-up by `min_margin`; accepted
    or not, it enters a ring of `vote` windows (default: the decoder's) with weight 1 (weight='count') or a weight that grows
    with its margin (weight='margin').  The candidate is the class with the largest weight in the ring among those with at
    least `min_votes` accepted windows there, or none.  A new grasp becomes the command after it has been the candidate for
    `dwell` windows in a row, none after `release` windows in a row (release=0: a grasp is never released, only replaced).

    min_cosine: one float, or {class id: float} with `default` for the ids it does not name (`thresholds_from_logits` makes
    one from a cued recording).  With the defaults every gate is open and `command` equals the decoder's `voted` bit for bit.

    The gate follows the decoder: a new `class_ids` object (set_classes, enroll, refresh) is installed before the next launch
    -- the ring empties and the command survives if its class id does -- and a push or reset of the decoder behind the gate's
    back makes the next `push` raise `CpNativeError` before anything is enqueued."""

    def __init__(self, decoder, min_cosine=-2.0, min_margin: float = 0.0, min_votes: int = 1, dwell: int = 1, release: int = 1,
                 weight: str = "count", vote: Optional[int] = None, default: float = -2.0):
        for name in ("class_ids", "n_seen", "vote", "push"):
            if not hasattr(decoder, name):
                raise TypeError("CommandGate wraps an OnlineDecoder, MultiStreamDecoder or AdaptiveMultiStreamDecoder")
        self.decoder = decoder
        self.multi = isinstance(decoder.class_ids, (list, tuple))
        self.n_streams = len(decoder.class_ids) if self.multi else 1
        vote = decoder.vote if vote is None else vote
        if not 1 <= int(vote) <= _lib.CP_ONLINE_MAX_VOTE:
            raise ValueError(f"vote must lie in 1..{_lib.CP_ONLINE_MAX_VOTE}")
        self.vote = int(vote)
        self._cfg = _lib.cp_online_gate_config()
        self._cfg.vote = self.vote
        self._cfg.min_votes, self._cfg.dwell, self._cfg.release, self._cfg.weight, self._cfg.min_margin = 1, 1, 1, 0, 0.0
        self.set(min_margin=min_margin, min_votes=min_votes, dwell=dwell, release=release, weight=weight)
        spec = self._check_thresholds(min_cosine, default)
        self._thr = [spec] * self.n_streams
        self._ids_seen = [None] * self.n_streams            # the class_ids object each stream's gate was installed from
        self._k = [0] * self.n_streams
        self.device = getattr(decoder, "device", None)
        self.ws = None                                      # allocated with the first launch
        self._rows_cache = {}
        self._left = self._seen_now()

    # ------------------------------------------------------------------ settings
    def set(self, **kw):
        """Change min_margin, min_votes, dwell, release or weight from the next window on (vote is fixed at construction)."""
        c = self._cfg
        new = dict(min_margin=c.min_margin, min_votes=c.min_votes, dwell=c.dwell, release=c.release,
                   weight="margin" if c.weight else "count")
        for k, v in kw.items():
            if k == "vote":
                raise ValueError("vote is fixed at construction: the ring is laid out by it")
            if k not in new:
                raise TypeError(f"set() takes min_margin, min_votes, dwell, release and weight, not {k!r}")
            new[k] = v
        mm, mv, dw, rl, w = _gate_settings(new)
        c.min_margin, c.min_votes, c.dwell, c.release, c.weight = mm, mv, dw, rl, w

    def use(self, config: dict):
        """Apply one config of `sweep_gate` / `gate_grid` (a dict with CommandGate's keys): the settings through `set`, and
        `min_cosine` (with `default`), if it is there, through `set_thresholds` on every stream.  `vote` is fixed at construction:
        a config that names another one is refused.  Nothing changes if a value is refused."""
        extra = set(config) - set(_GATE_KEYS)
        if extra:
            raise ValueError(f"a gate config takes {', '.join(_GATE_KEYS)}, not {sorted(extra)[0]!r}")
        if "vote" in config and config["vote"] != self.vote:
            raise ValueError("vote is fixed at construction: the ring is laid out by it")
        if "default" in config and "min_cosine" not in config:
            raise ValueError("default goes with min_cosine")
        spec = self._check_thresholds(config["min_cosine"], config.get("default", -2.0)) if "min_cosine" in config else None
        self.set(**{k: v for k, v in config.items() if k not in ("vote", "min_cosine", "default")})
        if spec is not None:
            for s in range(self.n_streams):
                self._thr[s] = spec
                self._ids_seen[s] = None

    @staticmethod
    def _check_thresholds(min_cosine, default):
        d = float(default)
        if isinstance(min_cosine, dict):
            spec = {int(k): float(v) for k, v in min_cosine.items()}
        else:
            spec, d = {}, float(min_cosine)
        if any(np.isnan(v) for v in list(spec.values()) + [d]):
            raise ValueError("min_cosine must not be NaN")
        return spec, d

    def set_thresholds(self, *args, default: float = -2.0):
        """set_thresholds(min_cosine) on a single-stream decoder, set_thresholds(stream, min_cosine) on a multi-stream one:
        a float or {class id: float} with `default` for the other ids.  They go in with the next launch, as a new class list
        does: that stream's ring empties and its command stays."""
        if len(args) != (2 if self.multi else 1):
            raise TypeError("set_thresholds(stream, min_cosine) on a multi-stream decoder, set_thresholds(min_cosine) otherwise")
        s = 0
        if self.multi:
            s = args[0]
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < self.n_streams:
                raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {s!r}")
            s = int(s)
        self._thr[s] = self._check_thresholds(args[-1], default)
        self._ids_seen[s] = None

    # ------------------------------------------------------------------ the device side (one method per C entry)
    def _args(self):
        if self.ws is None:
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_gate_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return C.byref(self._cfg), self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_set_classes(self, s: int, ids: np.ndarray, thr: np.ndarray):
        k = int(ids.shape[0])
        args = self._args()
        _lib.check(self.lib.cp_online_gate_set_classes(*args, s, (C.c_int32 * k)(*ids.tolist()), (C.c_float * k)(*thr.tolist()), k,
                                                       self._stream()), "cp_online_gate_set_classes")

    def _dev_reset(self, s: int):
        args = self._args()
        _lib.check(self.lib.cp_online_gate_reset(*args, s, self._stream()), "cp_online_gate_reset")

    def _dev_push(self, logits_ptr: int, ldl: int, row0: np.ndarray, m: np.ndarray, rows: int):
        """one launch over `rows` packed rows -> (command, accepted) (2, rows) int32 and (conf, margin) (2, rows) f32"""
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.device)
        ca = torch.empty(2, rows, dtype=torch.int32, device=self.device)
        cm = torch.empty(2, rows, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.cp_online_gate_push(*args, logits_ptr, ldl, rm[0].data_ptr(), rm[1].data_ptr(), rows, ca[0].data_ptr(),
                                                ca[1].data_ptr(), cm[0].data_ptr(), cm[1].data_ptr(), self._stream()),
                   "cp_online_gate_push")
        return ca, cm

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
                raise ValueError("the gate takes 1..64 ascending class ids in 0..2**31-2 (-1 is its 'none')")
            spec, d = self._thr[s]
            thr = np.array([spec.get(int(i), d) for i in ids], dtype=np.float32)
            self._dev_set_classes(s, ids, thr)
            self._ids_seen[s] = cur
            self._k[s] = int(ids.shape[0])

    def _check_in_step(self):
        if not np.array_equal(self._seen_now(), self._left):
            raise _lib.CpNativeError("the decoder was pushed or reset behind the gate (its n_seen is not what the gate left): the "
                                     "gate's ring no longer follows the stream; push and reset through the gate, or reset() it")

    # ------------------------------------------------------------------ the gate over per-stream logits
    def _gate(self, per_stream, trusted: bool = False):
        """per_stream: n_streams entries, None or (M_s, K_s) f32 logits -> per stream (command, accepted, conf, margin).
        trusted: the entries are what the decoder's own push just returned (their layout is known, see _packed)."""
        self._sync_classes()
        step = _lib.CP_ONLINE_MAX_WINDOWS
        if trusted:
            ms = [0 if t is None else t.shape[0] for t in per_stream]
        else:
            ms = []
            for s, t in enumerate(per_stream):
                if t is None:
                    ms.append(0)
                    continue
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
                    raise ValueError("logits must be (M, K) float32 tensors")
                if t.shape[0] and self._ids_seen[s] is None:
                    raise _lib.CpNativeError(f"stream {s} has logits but no class list: set_classes on the decoder first")
                if t.shape[0] and t.shape[1] != self._k[s]:
                    raise ValueError(f"stream {s}: logits have {t.shape[1]} columns, its class list {self._k[s]} ids")
                ms.append(int(t.shape[0]))
        outs = []                                              # per round: per stream (command, accepted, conf, margin)
        for lo in range(0, max(max(ms), 1), step):
            m = np.array([min(max(n - lo, 0), step) for n in ms], dtype=np.int64)
            rows = int(m.sum())
            row0 = np.zeros_like(m)
            np.cumsum(m[:-1], out=row0[1:])
            if rows == 0:
                dev = next((t.device for t in per_stream if t is not None), self.device)
                ca, cm = torch.empty(2, 0, dtype=torch.int32, device=dev), torch.empty(2, 0, dtype=torch.float32, device=dev)
            else:
                whole = lo == 0 and max(ms) <= step
                views = [None if n == 0 else (per_stream[s] if whole else per_stream[s][lo:lo + n]) for s, n in enumerate(m.tolist())]
                base, ldl = self._packed(views, row0, trusted)
                ca, cm = self._dev_push(base.data_ptr(), ldl, row0, m, rows)
            if self.n_streams == 1:
                outs.append([(ca[0], ca[1], cm[0], cm[1])])
                continue
            ml = m.tolist()
            outs.append(list(zip(ca[0].split(ml), ca[1].split(ml), cm[0].split(ml), cm[1].split(ml))))
        if len(outs) == 1:
            return outs[0]
        return [tuple(torch.cat([o[s][i] for o in outs]) for i in range(4)) for s in range(self.n_streams)]

    @staticmethod
    def _packed(views, row0, trusted: bool = False):
        """the logits of one launch as (tensor whose data_ptr is row 0, leading dimension), see _packed_rows"""
        return _packed_rows(views, row0, trusted, MAX_CLASSES)

    # ------------------------------------------------------------------ API
    def apply(self, logits):
        """The gate alone on logits the caller already has (of the decoder's next windows, in order): (M, K) f32 on the GPU ->
        (command, accepted, conf, margin); on a multi-stream decoder a list with one entry per stream (None: no windows) -> one
        such tuple per stream.  command, accepted (M,) int32 class ids or -1; conf, margin (M,) f32."""
        if self.multi:
            if isinstance(logits, torch.Tensor) or len(logits) != self.n_streams:
                raise ValueError(f"logits must be a sequence of {self.n_streams} entries (None or (M, K) tensors)")
            out = self._gate(list(logits))
        else:
            out = self._gate([logits])[0]
        self._left = self._seen_now()
        return out

    def _extend(self, res, gated, return_logits: bool):
        keep = [x for i, x in enumerate(res) if i != 2 or return_logits]
        return tuple(keep) + tuple(gated)

    def push(self, raw, return_logits: bool = False, return_windows: bool = False):
        """What the decoder's `push` takes (raw (n, 12), or one chunk per stream) -> the decoder's tuple(s) extended by
        command, accepted, conf, margin: (pred, voted[, logits][, windows], command, accepted, conf, margin)."""
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
            gated = self._gate([r[2] for r in res], trusted=True)
            return [self._extend(r, g, return_logits) for r, g in zip(res, gated)]
        return self._extend(res, self._gate([res[2]], trusted=True)[0], return_logits)

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back (this waits for the device; a test and debugging aid):
        command (class id or -1), pending (class slot, -1 for none, or None if nothing is pending), run, and ring, the
        (slot or -1, weight) entries from the oldest to the newest.  The layout is that of OgState (csrc/online_gate.cuh):
        int32 K, head, len, command + 1, pending, run, 2 unused, ids[64], f32 min_cosine[64], int32 ring slots [256] and ring
        weights [256]."""
        if isinstance(stream, bool) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must lie in 0..{self.n_streams - 1}")
        if self.ws is None:
            return dict(command=-1, pending=None, run=0, ring=[])
        per = 8 + 2 * MAX_CLASSES + 2 * _lib.CP_ONLINE_MAX_VOTE
        w = self.ws[:self.n_streams * per * 4].view(torch.int32).reshape(self.n_streams, per)[int(stream)].cpu().numpy()
        head, n, run = int(w[1]), int(w[2]), int(w[5])
        slots, weights = w[8 + 2 * MAX_CLASSES:][:_lib.CP_ONLINE_MAX_VOTE], w[8 + 2 * MAX_CLASSES + _lib.CP_ONLINE_MAX_VOTE:]
        at = [(head - n + i) % self.vote for i in range(n)]
        return dict(command=int(w[3]) - 1, pending=int(w[4]) if run else None, run=run,
                    ring=[(int(slots[i]), int(weights[i])) for i in at])

    def reset(self, streams=None):
        """Reset the decoder and the gate (ring, pending state and command to none; classes and thresholds stay); on a
        multi-stream decoder the listed streams, default all."""
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
# grasp drive: a proportional level and the electrodes' health per window (cp_online_drive_*)
# ---------------------------------------------------------------------------------------------------------------------------
DRIVE_ONE = _lib.CP_ONLINE_DRIVE_ONE    # full level: levels are integers out of 4096
_DRIVE_LEVELS = ("on_level", "off_level", "rise", "fall")
_DRIVE_COUNTS = ("bad_after", "good_after")
_DRIVE_FOLLOW = ("pred", "voted", "command")
_OD_WORDS = 8 + 16 + MAX_CLASSES + 48 + MAX_CLASSES * EMG_DIM + MAX_CLASSES * EMG_DIM // 4 + _lib.CP_ONLINE_DRIVE_MAX_SMOOTH
_OD_RING = _OD_WORDS - _lib.CP_ONLINE_DRIVE_MAX_SMOOTH


def _drive_settings(new: dict):
    """on_level, off_level, rise, fall (fractions of full level) and bad_after, good_after as the C config takes them, or
    ValueError"""
    out = []
    for k in _DRIVE_LEVELS:
        v = new[k]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{k} must be a fraction in 0..1")
        out.append(int(np.rint(float(v) * DRIVE_ONE)))
    if out[1] > out[0]:
        raise ValueError("off_level must not exceed on_level")
    if out[2] < 1 or out[3] < 1:
        raise ValueError(f"rise and fall must be at least 1/{DRIVE_ONE}")
    for k in _DRIVE_COUNTS:
        v = new[k]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 65535:
            raise ValueError(f"{k} must be an int in 1..65535")
        out.append(int(v))
    return out


def _check_profile(profile: dict) -> dict:
    """a profile (see drive_profile) as the arrays cp_online_drive_set_profile takes, or ValueError"""
    missing = [k for k in ("ids", "rest", "span", "weight", "low", "high") if k not in profile]
    if missing:
        raise ValueError(f"a drive profile holds ids, rest, span, weight, low and high; {missing[0]!r} is missing")
    ids = _ids_array(profile["ids"])
    k = ids.shape[0]
    chan = {n: np.ascontiguousarray(np.asarray(profile[n], dtype=np.float32).reshape(-1)) for n in ("rest", "low", "high")}
    span = np.ascontiguousarray(np.asarray(profile["span"], dtype=np.float32))
    weight = np.asarray(profile["weight"])
    if any(v.shape != (EMG_DIM,) for v in chan.values()) or span.shape != (k, EMG_DIM) or weight.shape != (k, EMG_DIM):
        raise ValueError(f"rest, low, high: ({EMG_DIM},); span, weight: ({k}, {EMG_DIM})")
    if not np.isfinite(chan["rest"]).all():
        raise ValueError("rest must be finite")
    if np.isnan(chan["low"]).any() or np.isnan(chan["high"]).any() or (chan["low"] > chan["high"]).any():
        raise ValueError("low and high must not be NaN, low <= high")
    if weight.dtype.kind not in "iu" or (weight < 0).any() or (weight > 255).any():
        raise ValueError("weight must hold integers in 0..255")
    return dict(ids=ids.astype(np.int32), span=span, weight=np.ascontiguousarray(weight.astype(np.int32)), **chan)


class GraspDrive(_OnStream):
    """How hard, next to which grasp: per stream one state machine on the device that reads the normalised windows of every
    push and the class the hand follows (include/cpnative.h, cp_online_drive_*; one launch more per push, nothing is copied to
    the host), and reports per window a proportional level `drive` in 0..1, whether the stream is `active`, and `bad`, the mask
    of electrodes whose windows have left their plausible range.

    source: a `CommandGate` (the drive follows its `command`) or any of the four decoders (it follows `voted`);
    follow='pred' | 'voted' | 'command' overrides that.  The level of a window is the weighted mean over the class's channels
    of (x - rest) / span, clamped to 0..1, over the channels that are good; it is averaged over the last `smooth` windows,
    switches the stream on at `on_level` and off below `off_level`, and moves by at most `rise` up and `fall` down per window.
    A channel is bad after `bad_after` windows in a row outside [low, high] and good again after `good_after` inside.  Levels
    are fractions of full level and are kept as integers out of 4096.  With smooth=1, on_level=off_level=0, rise=fall=1 and an
    open range `drive` is the level of each window on its own.

    profile: what `drive_profile` returns (a dict with ids, rest, span, weight, low, high); on a multi-stream source one for
    every stream, or a list with one (or None) per stream.  A class id that is not in the profile drives nothing.  A push or
    reset of the source behind the drive's back makes the next `push` raise `CpNativeError` before anything is enqueued."""

    def __init__(self, source, profile=None, smooth: int = 10, on_level: float = 0.08, off_level: float = 0.04, rise: float = 1.0,
                 fall: float = 1.0, bad_after: int = 20, good_after: int = 100, follow: Optional[str] = None):
        self.gate = source if isinstance(source, CommandGate) else None
        self.source = source
        self.decoder = source.decoder if self.gate is not None else source
        for name in ("class_ids", "n_seen", "push"):
            if not hasattr(self.decoder, name):
                raise TypeError("GraspDrive wraps a CommandGate, an OnlineDecoder, MultiStreamDecoder or AdaptiveMultiStreamDecoder")
        if follow is None:
            follow = "command" if self.gate is not None else "voted"
        if follow not in _DRIVE_FOLLOW:
            raise ValueError("follow must be 'pred', 'voted' or 'command'")
        if follow == "command" and self.gate is None:
            raise ValueError("follow='command' takes a CommandGate as the source")
        self.follow = follow
        self.multi = isinstance(self.decoder.class_ids, (list, tuple))
        self.n_streams = len(self.decoder.class_ids) if self.multi else 1
        if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or not 1 <= int(smooth) <= _lib.CP_ONLINE_DRIVE_MAX_SMOOTH:
            raise ValueError(f"smooth must be an int in 1..{_lib.CP_ONLINE_DRIVE_MAX_SMOOTH}")
        self.smooth = int(smooth)
        self._cfg = _lib.cp_online_drive_config()
        self._cfg.smooth = self.smooth
        self._cfg.on_level = self._cfg.off_level = 0
        self._cfg.rise = self._cfg.fall = DRIVE_ONE
        self._cfg.bad_after = self._cfg.good_after = 1
        self.set(on_level=on_level, off_level=off_level, rise=rise, fall=fall, bad_after=bad_after, good_after=good_after)
        self.device = getattr(self.decoder, "device", None)
        self.ws = None                                      # allocated with the first launch
        self._rows_cache = {}
        self._profile = [None] * self.n_streams
        self._left = self._seen_now()
        if profile is not None:
            each = list(profile) if isinstance(profile, (list, tuple)) else [profile] * self.n_streams
            if len(each) != self.n_streams:
                raise ValueError(f"profile: one dict, or a list of {self.n_streams} (None: no profile yet)")
            for s, p in enumerate(each):
                if p is not None:
                    self._install(s, p)

    # ------------------------------------------------------------------ settings
    def set(self, **kw):
        """Change on_level, off_level, rise, fall, bad_after or good_after from the next window on (smooth is fixed at
        construction)."""
        c = self._cfg
        new = dict(on_level=c.on_level / DRIVE_ONE, off_level=c.off_level / DRIVE_ONE, rise=c.rise / DRIVE_ONE, fall=c.fall / DRIVE_ONE,
                   bad_after=c.bad_after, good_after=c.good_after)
        for k, v in kw.items():
            if k == "smooth":
                raise ValueError("smooth is fixed at construction: the ring is laid out by it")
            if k not in new:
                raise TypeError(f"set() takes on_level, off_level, rise, fall, bad_after and good_after, not {k!r}")
            new[k] = v
        c.on_level, c.off_level, c.rise, c.fall, c.bad_after, c.good_after = _drive_settings(new)

    def _index(self, stream) -> int:
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < self.n_streams:
            raise IndexError(f"stream index must be an int in 0..{self.n_streams - 1}, got {stream!r}")
        return int(stream)

    def set_profile(self, *args):
        """set_profile(profile) on a single-stream source, set_profile(stream, profile) on a multi-stream one.  That stream
        starts again: every channel good, the ring empty, inactive, drive 0."""
        if len(args) != (2 if self.multi else 1):
            raise TypeError("set_profile(stream, profile) on a multi-stream source, set_profile(profile) otherwise")
        self._install(self._index(args[0]) if self.multi else 0, args[-1])

    def _install(self, s: int, profile: dict):
        p = _check_profile(profile)
        self._dev_set_profile(s, p)
        self._profile[s] = p

    # ------------------------------------------------------------------ the device side (one method per C entry)
    def _args(self):
        if self.ws is None:
            self.lib = _lib.load()
            self.ws = torch.zeros(self.lib.cp_online_drive_workspace_bytes(self.n_streams), dtype=torch.uint8, device=self.device)
        return C.byref(self._cfg), self.n_streams, self.ws.data_ptr(), self.ws.numel()

    def _dev_set_profile(self, s: int, p: dict):
        args = self._args()
        f, i = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _lib.check(self.lib.cp_online_drive_set_profile(
            *args, s, p["ids"].ctypes.data_as(i), int(p["ids"].shape[0]), p["rest"].ctypes.data_as(f), p["span"].ctypes.data_as(f),
            p["weight"].ctypes.data_as(i), p["low"].ctypes.data_as(f), p["high"].ctypes.data_as(f), self._stream()),
            "cp_online_drive_set_profile")

    def _dev_reset(self, s: int):
        args = self._args()
        _lib.check(self.lib.cp_online_drive_reset(*args, s, self._stream()), "cp_online_drive_reset")

    def _dev_push(self, windows_ptr: int, ldw: int, cls_ptr: int, row0: np.ndarray, m: np.ndarray, rows: int):
        """one launch over `rows` packed rows -> drive (rows,) f32 and (active, bad) (2, rows) int32"""
        args = self._args()
        rm = _rows_on_device(self._rows_cache, row0, m, self._stream(), self.device)
        drive = torch.empty(rows, dtype=torch.float32, device=self.device)
        ab = torch.empty(2, rows, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.cp_online_drive_push(*args, windows_ptr, ldw, cls_ptr, rm[0].data_ptr(), rm[1].data_ptr(), rows,
                                                 drive.data_ptr(), ab[0].data_ptr(), ab[1].data_ptr(), self._stream()),
                   "cp_online_drive_push")
        return drive, ab

    # ------------------------------------------------------------------ staying in step with the source
    def _seen_now(self) -> np.ndarray:
        return np.array(self.decoder.n_seen, dtype=np.int64).reshape(-1).copy()

    def _check_in_step(self):
        if not np.array_equal(self._seen_now(), self._left):
            raise _lib.CpNativeError("the source was pushed or reset behind the drive (its n_seen is not what the drive left): the "
                                     "drive's ring no longer follows the stream; push and reset through the drive, or reset() it")

    def _check_profiles(self, has_rows):
        for s, rows in enumerate(has_rows):
            if rows and self._profile[s] is None:
                raise _lib.CpNativeError(f"stream {s} has windows but no drive profile: set_profile first")

    # ------------------------------------------------------------------ the drive over per-stream windows and classes
    def _drive(self, wins, cls, trusted: bool = False):
        """wins, cls: n_streams entries, None or (M_s, 12) f32 windows and (M_s,) int32 class ids -> per stream (drive,
        active, bad).  trusted: the entries are what the source's own push just returned (their layout is known)."""
        step = _lib.CP_ONLINE_MAX_WINDOWS
        ms = []
        for s, (w, c) in enumerate(zip(wins, cls)):
            if w is None or c is None:
                if w is not None or c is not None:
                    raise ValueError(f"stream {s}: windows and cls go together")
                ms.append(0)
                continue
            if not trusted:
                if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != EMG_DIM \
                        or w.device.type != "cuda":
                    raise ValueError("windows must be (M, 12) float32 tensors on the GPU")
                if not isinstance(c, torch.Tensor) or c.dtype != torch.int32 or c.dim() != 1 or c.shape[0] != w.shape[0] \
                        or c.device != w.device:
                    raise ValueError("cls must be (M,) int32 tensors next to their windows")
            ms.append(int(w.shape[0]))
        self._check_profiles(ms)
        outs = []                                              # per round: per stream (drive, active, bad)
        for lo in range(0, max(max(ms), 1), step):
            m = np.array([min(max(n - lo, 0), step) for n in ms], dtype=np.int64)
            rows = int(m.sum())
            row0 = np.zeros_like(m)
            np.cumsum(m[:-1], out=row0[1:])
            if rows == 0:
                dev = next((t.device for t in wins if t is not None), self.device)
                drive, ab = torch.empty(0, dtype=torch.float32, device=dev), torch.empty(2, 0, dtype=torch.int32, device=dev)
            else:
                whole = lo == 0 and max(ms) <= step
                ml = m.tolist()
                wv = [None if n == 0 else (wins[s] if whole else wins[s][lo:lo + n]) for s, n in enumerate(ml)]
                cv = [None if n == 0 else (cls[s] if whole else cls[s][lo:lo + n]).unsqueeze(1) for s, n in enumerate(ml)]
                wbase, ldw = _packed_rows(wv, row0, trusted, EMG_DIM)
                cbase, ldc = _packed_rows(cv, row0, trusted, 1)
                if ldc != 1:                                   # (a class id every ldc words: not what the entry takes)
                    cbase = torch.cat([v for v in cv if v is not None])
                drive, ab = self._dev_push(wbase.data_ptr(), ldw, cbase.data_ptr(), row0, m, rows)
            if self.n_streams == 1:
                outs.append([(drive, ab[0], ab[1])])
                continue
            ml = m.tolist()
            outs.append(list(zip(drive.split(ml), ab[0].split(ml), ab[1].split(ml))))
        if len(outs) == 1:
            return outs[0]
        return [tuple(torch.cat([o[s][i] for o in outs]) for i in range(3)) for s in range(self.n_streams)]

    # ------------------------------------------------------------------ API
    def apply(self, windows, cls):
        """The drive alone on tensors the caller already has (of the source's next windows, in order): windows (M, 12) f32 and
        cls (M,) int32 (class ids, -1: none) on the GPU -> (drive, active, bad); on a multi-stream source lists with one entry
        per stream (None: no windows) -> one such tuple per stream.  drive (M,) f32 in 0..1, active (M,) int32 0/1, bad (M,)
        int32, bit c set while channel c is bad."""
        if self.multi:
            if isinstance(windows, torch.Tensor) or isinstance(cls, torch.Tensor) or len(windows) != self.n_streams \
                    or len(cls) != self.n_streams:
                raise ValueError(f"windows and cls must be sequences of {self.n_streams} entries (None or tensors)")
            out = self._drive(list(windows), list(cls))
        else:
            out = self._drive([windows], [cls])[0]
        self._left = self._seen_now()
        return out

    def _class_index(self, return_logits: bool) -> int:
        """where the class the drive follows sits in the source's tuple (windows asked for)"""
        return {"pred": 0, "voted": 1, "command": 3 + int(return_logits)}[self.follow]

    def _strip(self, res, driven, return_logits: bool, return_windows: bool):
        at = 2 + int(return_logits)                            # where the windows sit
        keep = [x for i, x in enumerate(res) if i != at or return_windows]
        return tuple(keep) + tuple(driven)

    def push(self, raw, return_logits: bool = False, return_windows: bool = False):
        """What the source's `push` takes (raw (n, 12), or one chunk per stream) -> the source's tuple(s) extended by drive,
        active, bad: behind a gate (pred, voted[, logits][, windows], command, accepted, conf, margin, drive, active, bad)."""
        self._check_in_step()
        if self.multi:
            if isinstance(raw, torch.Tensor) or len(raw) != self.n_streams:
                raise ValueError(f"chunks must be a sequence of {self.n_streams} entries (None or (n, 12) tensors)")
            self._check_profiles([c is not None and c.shape[0] > 0 for c in raw])
        else:
            self._check_profiles([True])
        res = self.source.push(raw, return_logits=return_logits, return_windows=True)
        return self._finish(res, return_logits, return_windows)

    def push_packed(self, raw, counts, return_logits: bool = False, return_windows: bool = False):
        """`push` for samples packed in stream order, as the multi-stream decoders' `push_packed`."""
        if not self.multi:
            raise TypeError("push_packed belongs to the multi-stream decoders")
        self._check_in_step()
        cnt = np.asarray(counts).reshape(-1)
        if cnt.shape[0] == self.n_streams:
            self._check_profiles((cnt > 0).tolist())
        res = self.source.push_packed(raw, counts, return_logits=return_logits, return_windows=True)
        return self._finish(res, return_logits, return_windows)

    def _finish(self, res, return_logits: bool, return_windows: bool):
        self._left = self._seen_now()
        at, ci = 2 + int(return_logits), self._class_index(return_logits)
        if self.multi:
            driven = self._drive([r[at] for r in res], [r[ci] for r in res], trusted=True)
            return [self._strip(r, d, return_logits, return_windows) for r, d in zip(res, driven)]
        return self._strip(res, self._drive([res[at]], [res[ci]], trusted=True)[0], return_logits, return_windows)

    def state(self, stream: int = 0) -> dict:
        """One stream's state as the device holds it, read back (this waits for the device; a test and debugging aid): out
        (the level, an integer out of 4096), active (0 / 1), bad (the mask), run (the 12 run counters) and ring, the raw
        levels from the oldest to the newest.  The layout is that of OdState (csrc/online_drive.cuh): int32 K, head, len,
        active, out, bad, 2 unused, run[16], ids[64], f32 rest[16], low[16], high[16], span[64][12], uint8 weight[64][12],
        int32 ring[256]."""
        s = self._index(stream)
        if self.ws is None:
            return dict(out=0, active=0, bad=0, run=[0] * EMG_DIM, ring=[])
        w = self.ws[:self.n_streams * _OD_WORDS * 4].view(torch.int32).reshape(self.n_streams, _OD_WORDS)[s].cpu().numpy()
        head, n = int(w[1]), int(w[2])
        ring = w[_OD_RING:]
        return dict(out=int(w[4]), active=int(w[3]), bad=int(w[5]), run=[int(x) for x in w[8:8 + EMG_DIM]],
                    ring=[int(ring[(head - n + i) % self.smooth]) for i in range(n)])

    def reset(self, streams=None):
        """Reset the source (a gate resets its decoder) and the drive (every channel good, ring empty, inactive, drive 0;
        the profiles stay); on a multi-stream source the listed streams, default all."""
        if self.multi and streams is not None:
            idx = sorted({self._index(s) for s in streams})
            self.source.reset(idx)
            for s in idx:
                self._dev_reset(s)
        else:
            self.source.reset()
            self._dev_reset(-1)
        self._left = self._seen_now()


def drive_profile(windows, expected, ids, level: float = 0.9, floor=None, min_windows: int = 25, headroom: float = 4.0) -> dict:
    """The profile of a `GraspDrive` from a cued recording: windows (N, 12), the normalised windows of the recording
    (`recording_windows`), and expected (N,), what the cue asked of each (`expected_commands`: a class id, REST or IGNORE).
    Host only (numpy).  Returns a dict of
      ids     the class ids, ascending;
      rest    (12,) the per-channel median over the REST windows;
      span    (K, 12) the per-channel `level` quantile over the windows cued for class k, minus rest; 0 for a class with fewer
              than `min_windows` windows (it drives nothing);
      weight  (K, 12) int32 rint(255 max(span, 0) / max_c span): how much of the class's effort a channel carries;
      high    (12,) rest + headroom (max seen - rest): above this a channel is not plausible;
      low     (12,) halfway between `floor` and the lowest value seen; floor is the value of a silent electrode, -mean / std
              per channel (one value or 12); None: -inf, the range is open below."""
    cid = _ids_array(ids)
    w = np.asarray(windows.detach().cpu() if isinstance(windows, torch.Tensor) else windows, dtype=np.float64)
    e = np.asarray(expected.detach().cpu() if isinstance(expected, torch.Tensor) else expected).reshape(-1)
    if w.ndim != 2 or w.shape[1] != EMG_DIM or e.shape[0] != w.shape[0]:
        raise ValueError(f"windows (N, {EMG_DIM}) and expected (N,) go together")
    if not 0.0 < float(level) <= 1.0:
        raise ValueError("level must lie in (0, 1]")
    if not float(headroom) >= 1.0:
        raise ValueError("headroom must be at least 1")
    at_rest = w[e == REST]
    if at_rest.shape[0] == 0:
        raise ValueError("the recording has no REST windows: the resting level is taken from them")
    rest = np.median(at_rest, axis=0)
    span = np.zeros((cid.shape[0], EMG_DIM))
    for k, c in enumerate(cid):
        rows = w[e == c]
        if rows.shape[0] >= max(int(min_windows), 1):
            span[k] = np.quantile(rows, float(level), axis=0) - rest
    top = span.max(axis=1, keepdims=True)
    weight = np.where(top > 0, np.rint(255.0 * np.maximum(span, 0.0) / np.where(top > 0, top, 1.0)), 0.0).astype(np.int32)
    seen = w[e != IGNORE] if (e != IGNORE).any() else w
    high = rest + float(headroom) * (seen.max(axis=0) - rest)
    if floor is None:
        low = np.full(EMG_DIM, -np.inf)
    else:
        low = 0.5 * (np.broadcast_to(np.asarray(floor, dtype=np.float64).reshape(-1), (EMG_DIM,)) + seen.min(axis=0))
    f = np.float32
    return dict(ids=cid, rest=rest.astype(f), span=span.astype(f), weight=weight, low=low.astype(f), high=high.astype(f))


# ---------------------------------------------------------------------------------------------------------------------------
# gate sweep: many CommandGate settings over one cued recording, scored on the device (cp_online_gate_sweep)
# ---------------------------------------------------------------------------------------------------------------------------
REST = -1                               # expected: the hand should do nothing
IGNORE = -2                             # expected: the window is not scored
SCORE_KEYS = ("n_cue", "n_rest", "hit", "wrong", "false_active", "switches", "segments", "reached", "latency_sum",
              "wrong_segments")


def _ids_array(ids) -> np.ndarray:
    cid = np.asarray(ids.detach().cpu() if isinstance(ids, torch.Tensor) else ids).reshape(-1)
    if cid.dtype.kind not in "iu" or not 1 <= cid.shape[0] <= MAX_CLASSES:
        raise ValueError(f"ids must hold 1..{MAX_CLASSES} integer class ids")
    cid = cid.astype(np.int64)
    if (np.diff(cid) <= 0).any() or cid[0] < 0 or cid[-1] >= 2 ** 31 - 1:
        raise ValueError("ids must be ascending, distinct and in 0..2**31-2")
    return cid


def expected_commands(labels, ids, phase: int = 0, rest=None) -> np.ndarray:
    """What the cue asks of each window of a recording with one label per raw sample (`window_labels(labels, phase)`): the
    class id if the window's label is one of `ids`, REST if it is `rest` (the label that means "do nothing"; None: there is no
    such label), IGNORE for a mixed or unlabelled window and for any other label.  (K_w,) int64; host only (numpy)."""
    cid = _ids_array(ids)
    wl = window_labels(labels, phase)
    out = np.full(wl.shape, IGNORE, dtype=np.int64)
    known = (wl >= 0) & np.isin(wl, cid)
    out[known] = wl[known]
    if rest is not None:
        out[(wl >= 0) & (wl == int(rest))] = REST
    return out


def score_commands(command, expected) -> dict:
    """The score of a command sequence against the cues; this function is its definition (the sweep kernel restates it).
    command (M,): class ids or -1 for none; expected (M,): class ids, REST or IGNORE.  With command[-1] = -1 and a segment a
    maximal run of consecutive windows with the same expected >= 0 (any other value ends it), all integers:
    n_cue            windows with expected >= 0
    n_rest           windows with expected == REST
    hit              cue windows with command == expected
    wrong            cue windows with command >= 0 and command != expected
    false_active     rest windows with command != -1
    switches         windows (all of them) with command[j] != command[j-1]
    segments         number of segments
    reached          segments with at least one hit
    latency_sum      over reached segments, index of the first hit - index of the segment's first window
    wrong_segments   segments with at least one wrong window
    Host only (numpy)."""
    cmd = np.asarray(command.detach().cpu() if isinstance(command, torch.Tensor) else command).astype(np.int64).reshape(-1)
    exp = np.asarray(expected.detach().cpu() if isinstance(expected, torch.Tensor) else expected).astype(np.int64).reshape(-1)
    if cmd.shape != exp.shape:
        raise ValueError("command and expected must hold one entry per window each")
    cue, rest = exp >= 0, exp == REST
    is_hit = cue & (cmd == exp)
    is_wrong = cue & (cmd >= 0) & (cmd != exp)
    prev_cmd = np.concatenate([[-1], cmd[:-1]])
    prev_exp = np.concatenate([[IGNORE], exp[:-1]])
    start = np.nonzero(cue & (exp != prev_exp))[0]                   # the first window of every segment
    seg = np.cumsum(cue & (exp != prev_exp)) - 1                     # the segment a cue window lies in
    n_seg = int(start.shape[0])
    first_hit = np.full(n_seg, -1, dtype=np.int64)
    hits = np.nonzero(is_hit)[0]
    first_hit[seg[hits][::-1]] = hits[::-1]                          # (the earliest hit is written last)
    reached = first_hit >= 0
    out = dict(n_cue=cue.sum(), n_rest=rest.sum(), hit=is_hit.sum(), wrong=is_wrong.sum(),
               false_active=(rest & (cmd != -1)).sum(), switches=(cmd != prev_cmd).sum(), segments=n_seg, reached=reached.sum(),
               latency_sum=(first_hit - start)[reached].sum(), wrong_segments=np.unique(seg[is_wrong]).shape[0])
    assert tuple(out) == SCORE_KEYS
    return {k: int(v) for k, v in out.items()}


def pick_gate(scores, max_false_rate: float = 0.02, max_wrong_rate: float = 0.05):
    """The index of the config to use, from the scores of `sweep_gate` (a dict of (G,) arrays): among the configs with
    false_active / n_rest <= max_false_rate and wrong / n_cue <= max_wrong_rate (a rate with a zero denominator is 0) the one with
    the most hits, then the smallest latency_sum / max(reached, 1), then the smallest index; None if no config is eligible."""
    sc = {k: np.asarray(scores[k], dtype=np.int64).reshape(-1) for k in SCORE_KEYS}

    def rate(num, den):
        return np.where(den > 0, num / np.maximum(den, 1), 0.0)

    ok = (rate(sc["false_active"], sc["n_rest"]) <= max_false_rate) & (rate(sc["wrong"], sc["n_cue"]) <= max_wrong_rate)
    if not ok.any():
        return None
    latency = sc["latency_sum"] / np.maximum(sc["reached"], 1)
    idx = np.nonzero(ok)[0]
    return int(min(idx.tolist(), key=lambda g: (-int(sc["hit"][g]), float(latency[g]), g)))


def gate_grid(**lists) -> list:
    """The cartesian product of lists of CommandGate settings as a list of config dicts, the last name varying fastest:
    gate_grid(dwell=[1, 3], release=[0, 5]) -> [{dwell: 1, release: 0}, {dwell: 1, release: 5}, {dwell: 3, ...}, ...]."""
    import itertools
    extra = set(lists) - set(_GATE_KEYS)
    if extra:
        raise ValueError(f"a gate config takes {', '.join(_GATE_KEYS)}, not {sorted(extra)[0]!r}")
    names = list(lists)
    return [dict(zip(names, combo)) for combo in itertools.product(*(list(lists[n]) for n in names))]


def _sweep_configs(configs, cid: np.ndarray):
    """configs (dicts with CommandGate's keys) -> the device arrays' host images: (G, 6) int32 in the layout of
    cp_online_gate_config (min_margin as its f32 bits) and (G, 64) f32 thresholds per class slot.  ValueError as CommandGate raises."""
    configs = list(configs)
    if not 1 <= len(configs) <= _lib.CP_ONLINE_GATE_SWEEP_MAX_CONFIGS:
        raise ValueError(f"sweep_gate takes 1..{_lib.CP_ONLINE_GATE_SWEEP_MAX_CONFIGS} configs, got {len(configs)}")
    cfg = np.zeros((len(configs), 6), dtype=np.int32)
    thr = np.zeros((len(configs), MAX_CLASSES), dtype=np.float32)
    known = set(cid.tolist())
    for g, c in enumerate(configs):
        if not isinstance(c, dict):
            raise ValueError(f"config {g} is not a dict")
        extra = set(c) - set(_GATE_KEYS)
        if extra:
            raise ValueError(f"config {g}: a gate config takes {', '.join(_GATE_KEYS)}, not {sorted(extra, key=str)[0]!r}")
        new = dict(min_margin=0.0, min_votes=1, dwell=1, release=1, weight="count")
        new.update({k: c[k] for k in new if k in c})
        vote = c.get("vote", VOTE)
        if isinstance(vote, bool) or not isinstance(vote, (int, np.integer)) or not 1 <= int(vote) <= _lib.CP_ONLINE_MAX_VOTE:
            raise ValueError(f"vote must lie in 1..{_lib.CP_ONLINE_MAX_VOTE}")
        mm, mv, dw, rl, w = _gate_settings(new)
        spec, d = CommandGate._check_thresholds(c.get("min_cosine", -2.0), c.get("default", -2.0))
        stray = set(spec) - known
        if stray:
            raise ValueError(f"config {g}: min_cosine names class id {sorted(stray)[0]}, which is not among ids")
        cfg[g, :5] = int(vote), mv, dw, rl, w
        cfg[g, 5:].view(np.float32)[0] = mm
        thr[g, :cid.shape[0]] = [spec.get(int(i), d) for i in cid]
    return cfg, thr


def _cue_slots(logits, expected, cid: np.ndarray) -> np.ndarray:
    """the checks of a cued recording's logits (M, K) and expected (M,) against the ids -> expected as (M,) int32 class slots
    (REST and IGNORE as they are)"""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] != cid.shape[0]:
        raise ValueError("logits must be an (M, K) float32 tensor with one column per id")
    exp = np.asarray(expected.detach().cpu() if isinstance(expected, torch.Tensor) else expected)
    if exp.shape != (logits.shape[0],) or exp.dtype.kind not in "iu":
        raise ValueError(f"expected must hold one integer entry per window ({logits.shape[0]})")
    exp = exp.astype(np.int64)
    pos = np.minimum(np.searchsorted(cid, exp), cid.shape[0] - 1)
    if ((exp >= 0) & (cid[pos] != exp)).any() or (exp < IGNORE).any():
        raise ValueError("expected holds class ids among ids, REST or IGNORE")
    return np.where(exp >= 0, pos, exp).astype(np.int32)


def _sweep_dev(logits: torch.Tensor, slots: np.ndarray, k: int, cfg: np.ndarray, thr: np.ndarray, want_commands: bool):
    """the device side of `sweep_gate` (one call of cp_online_gate_sweep) -> scores (G, 10) int64 on the host, commands (G, M)
    int32 slots on the device or None"""
    lib = _lib.load()
    dev, m, g = logits.device, int(logits.shape[0]), int(cfg.shape[0])
    with torch.cuda.device(dev):
        exp_d = torch.from_numpy(slots).to(dev)
        cfg_d = torch.from_numpy(cfg).to(dev)
        thr_d = torch.from_numpy(thr).to(dev)
        scratch = torch.empty(lib.cp_online_gate_sweep_scratch_bytes(m), dtype=torch.uint8, device=dev)
        scores = torch.empty(g, _lib.CP_ONLINE_GATE_SCORES, dtype=torch.int64, device=dev)
        commands = torch.empty(g, m, dtype=torch.int32, device=dev) if want_commands else None
        _lib.check(lib.cp_online_gate_sweep(logits.data_ptr(), int(logits.stride(0)), m, k, exp_d.data_ptr(), cfg_d.data_ptr(),
                                            thr_d.data_ptr(), g, scratch.data_ptr(), scratch.numel(), scores.data_ptr(),
                                            commands.data_ptr() if want_commands else None,
                                            torch.cuda.current_stream(dev).cuda_stream), "cp_online_gate_sweep")
        return scores.cpu().numpy(), commands


def sweep_gate(logits, expected, ids, configs, return_commands: bool = False):
    """Score many CommandGate settings over one cued recording in one pass on the device (cp_online_gate_sweep: one wave per
    config, each from a fresh gate).  logits (M, K) f32 on the GPU, what `push(..., return_logits=True)` returned for the
    recording; expected (M,) as `expected_commands` gives it; ids the K ascending class ids of the columns; configs a sequence
    of dicts with CommandGate's keys (min_cosine: a float or {id: float} with `default`; min_margin, min_votes, dwell, release,
    weight, vote), missing keys at CommandGate's defaults (vote: 25), checked as CommandGate checks them before anything is
    enqueued.  Returns {key: (G,) int64 array} with the keys of `score_commands`: config g's entry is `score_commands` of the
    commands a fresh CommandGate with config g returns for these logits.  return_commands=True: (scores, commands) with
    commands (G, M) int32 on the GPU, class ids or -1.  One host synchronisation: the copy of the score table."""
    cid = _ids_array(ids)
    cfg, thr = _sweep_configs(configs, cid)
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
        scores, commands = _sweep_dev(logits, slots, int(cid.shape[0]), cfg, thr, return_commands)
    out = {k: scores[:, i].copy() for i, k in enumerate(SCORE_KEYS)}
    if not return_commands:
        return out
    if m and not np.array_equal(cid, np.arange(cid.shape[0])):        # slots -> class ids, a block of rows at a time
        table = torch.from_numpy(np.concatenate([[-1], cid]).astype(np.int32)).to(commands.device)
        step = max(1, (1 << 24) // m)
        for lo in range(0, g, step):
            commands[lo:lo + step] = table[(commands[lo:lo + step] + 1).long()]
    return out, commands


# ---------------------------------------------------------------------------------------------------------------------------
# grasp-set search: many class subsets of one cued recording, scored on the device (cp_online_subset_sweep)
# ---------------------------------------------------------------------------------------------------------------------------
SUBSET_SCORE_KEYS = ("n_cue", "hit", "voted_hit", "classes_scored", "worst_class", "worst_hit", "worst_n")
MAX_SUBSETS = _lib.CP_ONLINE_SUBSET_SWEEP_MAX_SUBSETS


def _check_vote(vote) -> int:
    if isinstance(vote, bool) or not isinstance(vote, (int, np.integer)) or not 1 <= int(vote) <= _lib.CP_ONLINE_MAX_VOTE:
        raise ValueError(f"vote must lie in 1..{_lib.CP_ONLINE_MAX_VOTE}")
    return int(vote)


def _mask_sizes(masks: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def _subset_masks(subsets, cid: np.ndarray) -> np.ndarray:
    """subsets (a sequence of collections of class ids, or a (G,) uint64 array of slot masks) -> (G,) uint64 slot masks, bit k =
    slot k of ids; ValueError for an id that is not among ids, an empty subset, a bit at or above K, and G outside
    1..MAX_SUBSETS"""
    k = int(cid.shape[0])
    if isinstance(subsets, np.ndarray) and subsets.dtype == np.uint64:
        if subsets.ndim != 1:
            raise ValueError("subsets as masks must be a (G,) uint64 array")
        masks = subsets.copy()
    else:
        subsets = list(subsets)
        masks = np.zeros(len(subsets), dtype=np.uint64)
        slot = {int(c): i for i, c in enumerate(cid)}
        for g, sub in enumerate(subsets):
            m = 0
            for c in (sub.tolist() if isinstance(sub, (np.ndarray, torch.Tensor)) else sub):
                if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or int(c) not in slot:
                    raise ValueError(f"subset {g} names {c!r}, which is not among ids")
                m |= 1 << slot[int(c)]
            masks[g] = m
    if not 1 <= masks.shape[0] <= MAX_SUBSETS:
        raise ValueError(f"sweep_subsets takes 1..{MAX_SUBSETS} subsets, got {masks.shape[0]}")
    if (masks == 0).any():
        raise ValueError(f"subset {int(np.nonzero(masks == 0)[0][0])} is empty")
    if k < 64 and (masks >> np.uint64(k)).any():
        raise ValueError(f"subset {int(np.nonzero(masks >> np.uint64(k))[0][0])} has a bit at or above the {k} class slots")
    return masks


def score_subset(logits, expected, ids, subset, vote: int = VOTE, per_class: bool = False):
    """What a user who keeps only the classes of `subset` gets out of a cued recording; this function is the definition (the
    subset sweep kernel restates it).  logits (M, K) f32 with one column per id; ids the K ascending class ids; expected (M,) as
    `expected_commands` gives it; subset a non-empty collection of ids among `ids`, S its set of slots.
    Kept rows: those with expected < 0 and those cued for a class of S.  Rows cued for another class are dropped, as though never
    recorded; kept rows with expected < 0 feed the ring and are not scored.
    Raw prediction of a kept row: the first maximum of its logits over the slots of S in ascending order (`>`, the lowest slot
    wins ties), or none if any of the row's K logits is not finite.
    Vote: the decoders' ring from an empty ring.  Every kept row's prediction enters (none takes a place without voting), the
    oldest leaves once `vote` are in; the voted prediction is the slot with the most entries, the smallest among equals, none if
    no slot has one.
    Returns, all ints, the keys of SUBSET_SCORE_KEYS and `size` (the number of classes of S):
    n_cue            kept rows cued for a class of S
    hit              of those, rows whose raw prediction is the cued class
    voted_hit        of those, rows whose voted prediction is the cued class
    classes_scored   classes of S with at least one cue row
    worst_class      the class id of S with the smallest voted recall voted_hit_c / n_c among those with n_c > 0 (fractions
                     compared by cross-multiplication, the smallest slot among equals); -1 if there is none
    worst_hit, worst_n   its voted_hit_c and n_c; 0, 0 if there is none
    per_class=True: (scores, (K,) int64 voted_hit_c per slot, 0 outside S).  Host only (numpy)."""
    cid = _ids_array(ids)
    vote = _check_vote(vote)
    lg = np.array(logits.detach().cpu() if isinstance(logits, torch.Tensor) else logits)
    slots = _cue_slots(torch.from_numpy(lg), expected, cid).astype(np.int64)
    mask = int(_subset_masks([subset], cid)[0])
    k = int(cid.shape[0])
    s_slots = np.array([i for i in range(k) if mask >> i & 1], dtype=np.int64)
    in_s = np.zeros(k, dtype=bool)
    in_s[s_slots] = True
    keep = (slots < 0) | in_s[np.maximum(slots, 0)]
    lg, e = lg[keep], slots[keep]
    n = int(e.shape[0])
    pred = np.where(np.isfinite(lg).all(axis=1), s_slots[np.argmax(lg[:, s_slots], axis=1)], -1) if n else np.zeros(0, np.int64)
    entered = np.zeros((n, k), dtype=np.int64)
    entered[np.nonzero(pred >= 0)[0], pred[pred >= 0]] = 1
    in_ring = np.cumsum(entered, axis=0)                              # per slot, entries among the last `vote` kept rows
    in_ring[vote:] -= in_ring[:-vote].copy()
    voted = np.where(in_ring.max(axis=1) > 0, in_ring.argmax(axis=1), -1) if n else np.zeros(0, np.int64)
    cue = e >= 0
    n_c = np.bincount(e[cue], minlength=k)
    hit_c = np.bincount(e[cue & (voted == e)], minlength=k)
    worst = -1
    for c in np.nonzero(n_c)[0].tolist():
        if worst < 0 or int(hit_c[c]) * int(n_c[worst]) < int(hit_c[worst]) * int(n_c[c]):
            worst = c
    out = dict(n_cue=cue.sum(), hit=(cue & (pred == e)).sum(), voted_hit=hit_c.sum(), classes_scored=np.count_nonzero(n_c),
               worst_class=cid[worst] if worst >= 0 else -1, worst_hit=hit_c[worst] if worst >= 0 else 0,
               worst_n=n_c[worst] if worst >= 0 else 0)
    assert tuple(out) == SUBSET_SCORE_KEYS
    out = {key: int(v) for key, v in out.items()}
    out["size"] = int(s_slots.shape[0])
    return (out, hit_c.astype(np.int64)) if per_class else out


def _subsets_dev(logits: torch.Tensor, slots: np.ndarray, k: int, masks: np.ndarray, vote: int, per_class: bool):
    """the device side of `sweep_subsets` (one call of cp_online_subset_sweep) -> scores (G, 7) int64 on the host (worst_class
    a slot), voted hits per class (G, 64) int32 on the device or None"""
    lib = _lib.load()
    dev, m, g = logits.device, int(logits.shape[0]), int(masks.shape[0])
    with torch.cuda.device(dev):
        exp_d = torch.from_numpy(slots).to(dev)
        masks_d = torch.from_numpy(masks.view(np.int64)).to(dev)
        scratch = torch.empty(lib.cp_online_subset_sweep_scratch_bytes(m), dtype=torch.uint8, device=dev)
        scores = torch.empty(g, _lib.CP_ONLINE_SUBSET_SCORES, dtype=torch.int64, device=dev)
        hits = torch.empty(g, MAX_CLASSES, dtype=torch.int32, device=dev) if per_class else None
        _lib.check(lib.cp_online_subset_sweep(logits.data_ptr(), int(logits.stride(0)), m, k, exp_d.data_ptr(), masks_d.data_ptr(),
                                              g, vote, scratch.data_ptr(), scratch.numel(), scores.data_ptr(),
                                              hits.data_ptr() if per_class else None,
                                              torch.cuda.current_stream(dev).cuda_stream), "cp_online_subset_sweep")
        return scores.cpu().numpy(), hits


def sweep_subsets(logits, expected, ids, subsets, vote: int = VOTE, per_class: bool = False):
    """Score many class subsets of one cued recording in one pass on the device (cp_online_subset_sweep: one wave per subset).
    logits (M, K) f32 on the GPU, what `push(..., return_logits=True)` returned for the recording; expected (M,) as
    `expected_commands` gives it; ids the K ascending class ids of the columns; subsets a sequence of collections of class ids,
    or a (G,) uint64 array of slot masks (bit k = ids[k]); vote the ring length.  Everything is checked before anything is
    enqueued: an id that is not among ids, an empty subset and more than MAX_SUBSETS subsets are refused with a ValueError.
    Returns {key: (G,) int64 array} with the keys of SUBSET_SCORE_KEYS and `size`: subset g's entry is `score_subset` of it
    (worst_class a class id).  per_class=True: (scores, hits) with hits (G, K) int32 on the GPU, voted_hit_c per slot.  M = 0:
    what `score_subset` gives for no rows (zeros, worst_class -1), without a launch.  One host synchronisation: the copy of the
    score table."""
    cid = _ids_array(ids)
    vote = _check_vote(vote)
    masks = _subset_masks(subsets, cid)
    slots = _cue_slots(logits, expected, cid)
    g, m, k = int(masks.shape[0]), int(logits.shape[0]), int(cid.shape[0])
    if m == 0:
        scores = np.zeros((g, len(SUBSET_SCORE_KEYS)), dtype=np.int64)
        scores[:, SUBSET_SCORE_KEYS.index("worst_class")] = -1
        hits = torch.zeros(g, MAX_CLASSES, dtype=torch.int32, device=logits.device) if per_class else None
    else:
        if logits.device.type != "cuda":
            raise ValueError("logits must be on the GPU")
        if logits.stride(1) != 1 or (m > 1 and logits.stride(0) < logits.shape[1]):
            logits = logits.contiguous()
        scores, hits = _subsets_dev(logits, slots, k, masks, vote, per_class)
    out = {key: scores[:, i].copy() for i, key in enumerate(SUBSET_SCORE_KEYS)}
    out["worst_class"] = np.where(out["worst_class"] >= 0, cid[np.clip(out["worst_class"], 0, k - 1)], -1)
    out["size"] = _mask_sizes(masks)
    return (out, hits[:, :k]) if per_class else out


def rank_subsets(scores) -> np.ndarray:
    """The order in which to prefer the subsets of one `sweep_subsets` table; this function is the policy's definition.  First
    the subsets every class of which has a cue row (classes_scored == size), then by larger worst_hit / max(worst_n, 1), then
    by larger voted_hit / max(n_cue, 1), then by larger hit / max(n_cue, 1) (float64 ratios), then by smaller index.
    Returns the (G,) int64 indices, best first.  Host only (numpy)."""
    sc = {key: np.asarray(scores[key], dtype=np.int64).reshape(-1) for key in SUBSET_SCORE_KEYS + ("size",)}
    cues = np.maximum(sc["n_cue"], 1)
    complete = sc["classes_scored"] == sc["size"]
    keys = (sc["hit"] / cues, sc["voted_hit"] / cues, sc["worst_hit"] / np.maximum(sc["worst_n"], 1), complete.astype(np.float64))
    # (lexsort: the last key first; it is stable, so equal subsets stay in index order)
    return np.lexsort(tuple(-key for key in keys)).astype(np.int64)


def _search_masks(k: int, score, min_size: int = 2, max_size=None, require: int = 0, exhaustive: int = 200_000, beam: int = 256,
                  keep: int = 8, max_call: int = MAX_SUBSETS) -> list:
    """The candidate generation of `search_grasp_sets` over slot masks of k slots; `score(masks (G,) uint64) -> scores` is what
    `sweep_subsets` returns for them and is called with at most max_call masks; require is a mask.  One record per size:
    dict(size, exhaustive, n_candidates, best=[(mask, {key: int})] in `rank_subsets` order)."""
    import itertools
    import math
    max_size = k if max_size is None else max_size
    for name, v in (("min_size", min_size), ("max_size", max_size), ("exhaustive", exhaustive), ("beam", beam), ("keep", keep)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} must be an int >= 1")
    n_req = bin(require).count("1")
    if not min_size <= max_size <= k:
        raise ValueError(f"sizes must satisfy min_size <= max_size <= {k} classes")
    if min_size < n_req:
        raise ValueError(f"min_size must be at least the {n_req} required classes")
    free = [i for i in range(k) if not require >> i & 1]
    bits = np.left_shift(np.uint64(1), np.arange(k, dtype=np.uint64))
    out, prev = [], None
    for size in range(int(min_size), int(max_size) + 1):
        complete = math.comb(k - n_req, size - n_req) <= exhaustive
        if complete:
            combos = list(itertools.combinations(free, size - n_req))
            combos = np.array(combos, dtype=np.uint64).reshape(len(combos), size - n_req)
            masks = np.left_shift(np.uint64(1), combos).sum(axis=1, dtype=np.uint64) | np.uint64(require)
        elif prev is None:
            raise ValueError(f"size {size} has more than exhaustive={exhaustive} candidates and there is no smaller size to extend")
        else:
            grown = prev[:beam, None] | bits[None, :]
            masks = np.unique(grown[(prev[:beam, None] & bits[None, :]) == 0])       # (ascending, each once)
        parts = [score(masks[lo:lo + max_call]) for lo in range(0, masks.shape[0], max_call)]
        sc = {key: np.concatenate([np.asarray(p[key]) for p in parts]) for key in SUBSET_SCORE_KEYS + ("size",)}
        order = rank_subsets(sc)
        out.append(dict(size=size, exhaustive=bool(complete), n_candidates=int(masks.shape[0]),
                        best=[(int(masks[g]), {key: int(sc[key][g]) for key in sc}) for g in order[:keep]]))
        prev = masks[order]
    return out


def search_grasp_sets(logits, expected, ids, min_size: int = 2, max_size=None, vote: int = VOTE, require=(),
                      exhaustive: int = 200_000, beam: int = 256, keep: int = 8) -> list:
    """Which grasps to keep: the best class subsets of every size min_size..max_size (None: all K) for a cued recording, by
    `rank_subsets` over `sweep_subsets`.  Sizes go in ascending order.  A size with at most `exhaustive` subsets that contain
    the ids of `require` is enumerated completely (in itertools.combinations order of slots); a larger size takes the one-class
    extensions of the previous size's best `beam` subsets, each once, in ascending mask order; ValueError if the first size is
    already too large.  Returns one record per size: dict(size, exhaustive (bool), n_candidates, best) with best the `keep`
    best as (ids tuple, scores dict) in rank order; the ids of a result are what `set_classes(ids=...)` takes."""
    cid = _ids_array(ids)
    vote = _check_vote(vote)
    _cue_slots(logits, expected, cid)
    require = tuple(require)
    need = int(_subset_masks([require], cid)[0]) if require else 0
    found = _search_masks(int(cid.shape[0]), lambda masks: sweep_subsets(logits, expected, cid, masks, vote), min_size, max_size,
                          need, exhaustive, beam, keep)
    for rec in found:
        rec["best"] = [(tuple(int(cid[i]) for i in range(cid.shape[0]) if mask >> i & 1), sc) for mask, sc in rec["best"]]
    return found


# ---------------------------------------------------------------------------------------------------------------------------
# electrode maps: candidates, the sweep that scores them on the device (cp_online_*map_sweep, csrc/online_maps.cuh), the pick
# ---------------------------------------------------------------------------------------------------------------------------
MAP_SCORE_KEYS = ("rows", "raw_hits", "voted_hits")
MAX_MAPS = _lib.CP_ONLINE_MAP_SWEEP_MAX_MAPS


def rotations(ring=(0, 1, 2, 3, 4, 5, 6, 7), reflect: bool = False) -> np.ndarray:
    """The maps of a sleeve that went back on turned around the forearm: (8, 12) int32, row s the ring shifted by s electrode
    positions (src[ring[i]] = ring[(i + s) % n]; row 0 is the identity), the other channels in place.  reflect=True adds the
    n mirrored ones (src[ring[i]] = ring[(s - i) % n]: the sleeve inside out or on the other arm), 16 rows.  The default ring
    is the Ninapro DB2 layout: electrodes 1-8 equally spaced around the forearm, 9-10 on flexor / extensor digitorum, 11-12
    on biceps / triceps; other sleeves pass their own ring, in order around the arm."""
    r = np.asarray(ring, dtype=np.int64).reshape(-1)
    n = r.shape[0]
    if n < 2 or len(set(r.tolist())) != n or r.min() < 0 or r.max() >= EMG_DIM:
        raise ValueError(f"ring: at least 2 distinct channels in 0..{EMG_DIM - 1}, in order around the arm")
    maps = []
    for mirror in ((False, True) if reflect else (False,)):
        for s in range(n):
            m = np.arange(EMG_DIM, dtype=np.int32)
            for i in range(n):
                m[r[i]] = r[(s - i) % n] if mirror else r[(i + s) % n]
            maps.append(m)
    return np.stack(maps)


def leave_one_out() -> np.ndarray:
    """The 12 maps that mask one electrode each: (12, 12) int32, row d the identity with src[d] = -1.  Scored with
    `score_channel_maps` they price a dead electrode before anything is masked."""
    m = np.tile(np.arange(EMG_DIM, dtype=np.int32), (EMG_DIM, 1))
    m[np.arange(EMG_DIM), np.arange(EMG_DIM)] = -1
    return m


def _sweep_target(decoder, stream):
    """(entry name, leading arguments, class ids (K,) int64, adaptive, calibrated) of the decoder (and stream) a sweep runs on"""
    if isinstance(decoder, _MultiStreamBase):
        if stream is None:
            raise ValueError("a multi-stream decoder needs stream=")
        s = decoder._index(stream)
        if not decoder._has_table[s]:
            raise _lib.CpNativeError(f"stream {s} has no class table: set_classes({s}, ...) first")
        name, lead = decoder._ENTRY + "_map_sweep", (*decoder._args(), s)
        if decoder._bank is not None:                          # the tail with the projection stream s decodes with
            name, lead = name + "_proj", (*lead, *decoder._bank_args())
        return (name, lead, decoder.class_ids[s].numpy().astype(np.int64), decoder._ENTRY.endswith("adapt"),
                decoder._enroll_calibrated(s))
    if isinstance(decoder, OnlineDecoder):
        if stream is not None:
            raise ValueError("stream= goes with a multi-stream decoder")
        if decoder.class_ids is None:
            raise _lib.CpNativeError("set_classes() first")
        adaptive = decoder.adapt is not None
        return ("cp_online_adapt_map_sweep" if adaptive else "cp_online_map_sweep", (C.byref(decoder._cfg), *decoder._ws()),
                decoder.class_ids.numpy().astype(np.int64), adaptive, decoder.calibrated)
    raise TypeError("score_channel_maps takes an OnlineDecoder, a MultiStreamDecoder or an AdaptiveMultiStreamDecoder")


def score_channel_maps(decoder, raw: torch.Tensor, labels, maps, fills=None, stream=None, return_pred: bool = False,
                       chunk_rows=None, per_class: bool = False):
    """Score many electrode maps over one cued recording in one pass on the device.  raw (n, 12) f32 on the GPU and labels (n,)
    are the recording `enroll` takes; maps (n_maps, 12) integers, one `set_channel_map` src per row (`rotations()`,
    `leave_one_out()`, your own); fills None (0.0) or (n_maps, 12).

    The definition, for map g: take a fresh stream of the same decoder -- same weights and class table, the vote ring empty,
    on the adaptive forms the current statistics frozen as `enroll` freezes them --, `set_channel_map(maps[g], fills[g])`,
    push the whole recording and count.  Returns one dict per map: rows (the windows whose `window_labels` class is in the
    decoder's table), raw_hits and voted_hits (of those, the windows whose pred / voted equals the cue), and with
    per_class=True per_class_voted_hits (K,) in the order of the decoder's class ids.  With return_pred=True returns
    (scores, pred, voted), pred and voted (n_maps, M) int32 class ids on the GPU.  The device pass reproduces the
    definition's pred and voted exactly; the decoder's live stream is not touched.

    The front end runs once for all maps (the un-normalised RMS series of the recording); rows (map, window) then run through
    the encoder in chunks of chunk_rows rows (default: sized to fill the chip), which the results do not depend on."""
    name, lead, ids, adaptive, calibrated = _sweep_target(decoder, stream)
    if not calibrated:
        raise _lib.CpNativeError("an AdaBN model has no BatchNorm statistics: calibrate() first")
    _check_raw(raw)
    lab = _sample_labels(labels, raw.shape[0])
    src = np.asarray(maps)
    if src.ndim != 2 or src.shape[1] != EMG_DIM or src.shape[0] < 1:
        raise ValueError(f"maps must be (n_maps, {EMG_DIM})")
    n_maps = src.shape[0]
    if n_maps > MAX_MAPS:
        raise ValueError(f"at most {MAX_MAPS} maps")
    fl = np.zeros((n_maps, EMG_DIM), dtype=np.float32) if fills is None else np.asarray(fills, dtype=np.float32)
    if fl.shape != (n_maps, EMG_DIM):
        raise ValueError(f"fills must be (n_maps, {EMG_DIM})")
    checked = [_check_map(src[g], fl[g]) for g in range(n_maps)]
    src32 = np.stack([c[0] for c in checked])
    fl32 = np.stack([c[1] for c in checked])
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("chunk_rows must be at least 1")
    wl = window_labels(lab, decoder.phase)
    M = wl.shape[0]
    if M < 1:
        raise ValueError("the recording completes no window")
    if n_maps * M >= 2 ** 31:
        raise ValueError("n_maps * windows must stay below 2**31")
    slot = np.searchsorted(ids, wl)
    slot = np.where((slot < ids.size) & (ids[np.minimum(slot, ids.size - 1)] == wl), slot, -1).astype(np.int32)
    # ---- everything is checked: from here on work is enqueued
    dev, lib = decoder.device, decoder.lib
    unit = torch.stack([torch.zeros(EMG_DIM, device=dev), torch.ones(EMG_DIM, device=dev)])
    rms = recording_windows(raw, unit, decoder._b, decoder._a, decoder.phase).contiguous()
    src_d, fill_d, slot_d = torch.as_tensor(src32).to(dev), torch.as_tensor(fl32).to(dev), torch.as_tensor(slot).to(dev)
    pred = torch.empty(n_maps, M, dtype=torch.int32, device=dev)
    voted = torch.empty(n_maps, M, dtype=torch.int32, device=dev) if return_pred else None
    scores = torch.zeros(n_maps, len(MAP_SCORE_KEYS), dtype=torch.int64, device=dev)
    hits = torch.zeros(n_maps, MAX_CLASSES, dtype=torch.int32, device=dev) if per_class else None
    chunk = 0 if chunk_rows is None else int(chunk_rows)
    scratch = torch.empty(lib.cp_online_map_sweep_scratch_bytes(n_maps * M, chunk, decoder._cfg.dtype, int(adaptive)),
                          dtype=torch.uint8, device=dev)
    _lib.check(getattr(lib, name)(*lead, rms.data_ptr(), M, decoder.mean_std.data_ptr(), src_d.data_ptr(), fill_d.data_ptr(), n_maps,
                                  int(ids.size), slot_d.data_ptr(), chunk, scratch.data_ptr(), scratch.numel(), pred.data_ptr(),
                                  voted.data_ptr() if voted is not None else None, scores.data_ptr(),
                                  hits.data_ptr() if hits is not None else None, decoder._stream()), name)
    sc = scores.cpu().numpy()
    hc = hits.cpu().numpy() if hits is not None else None
    out = []
    for g in range(n_maps):
        d = {k: int(v) for k, v in zip(MAP_SCORE_KEYS, sc[g])}
        if per_class:
            d["per_class_voted_hits"] = hc[g, :ids.size].astype(np.int64)
        out.append(d)
    return (out, pred, voted) if return_pred else out


def pick_channel_map(scores) -> int:
    """The index of the best map of `score_channel_maps`: the most voted hits, then the most raw hits, then the lowest index.
    The caller then calls `set_channel_map(maps[index], fills[index])`."""
    if len(scores) == 0:
        raise ValueError("no scores")
    return max(range(len(scores)), key=lambda g: (scores[g]["voted_hits"], scores[g]["raw_hits"], -g))
