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


def _engine_of(model_or_engine) -> Engine:
    e = getattr(model_or_engine, "engine", model_or_engine)
    if not isinstance(e, Engine):
        raise TypeError("OnlineDecoder takes a contrastiveprosthetics_amd Model or Engine")
    return e


class OnlineDecoder:
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
        if dtype is None:
            dtype = {CP_F32: "f32", CP_BF16: "bf16", CP_FP8: "fp8"}[e.dtype]
        if dtype == "fp8":
            raise _lib.CpNativeError("OnlineDecoder runs in 'f32' or 'bf16'; there is no 8-bit online path")
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        if e.specs["emg_net.last.0.weight"][0] != CP_D_E:
            raise _lib.CpNativeError(f"OnlineDecoder is built for d_e={CP_D_E}")
        if not 1 <= int(vote) <= _lib.CP_ONLINE_MAX_VOTE:
            raise ValueError(f"vote must lie in 1..{_lib.CP_ONLINE_MAX_VOTE}")
        if not 0 <= int(phase) < STRIDE:
            raise ValueError(f"phase must lie in 0..{STRIDE - 1}")
        if not 1 <= int(max_windows_per_push) <= _lib.CP_ONLINE_MAX_WINDOWS:
            raise ValueError(f"max_windows_per_push must lie in 1..{_lib.CP_ONLINE_MAX_WINDOWS}")
        if classes is not None:
            self._check_count(len(classes))
        if b is None:
            b, a = butter_bandpass()
        b = np.asarray(b, dtype=np.float64).reshape(-1)
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        if len(b) != len(a) or not 2 <= len(b) <= 17 or a[0] == 0.0:
            raise ValueError("b and a: 2..17 coefficients each, a[0] != 0")
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
        cfg = _lib.cp_online_config()
        cfg.dtype = CP_F32 if dtype == "f32" else CP_BF16
        cfg.max_windows = self.max_windows
        cfg.vote = self.vote
        cfg.phase = self.phase
        cfg.n_coef = len(b)
        for i in range(len(b)):
            cfg.b[i], cfg.a[i] = float(b[i]), float(a[i])
        self._cfg = cfg
        self.mean_std = torch.stack([self._channels(mean), self._channels(std)]).contiguous()
        nbytes = (self.lib.cp_online_workspace_bytes if adapt is None else self.lib.cp_online_adapt_workspace_bytes)(self.max_windows, cfg.dtype)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.n_seen = 0
        self.class_ids: Optional[torch.Tensor] = None
        self.refresh()
        if classes is not None:
            self.set_classes(classes)

    # ------------------------------------------------------------------ helpers
    def _channels(self, v) -> torch.Tensor:
        t = torch.as_tensor(v, dtype=torch.float32).to(self.device).reshape(-1)
        if t.numel() == 1:
            t = t.expand(EMG_DIM)
        if t.numel() != EMG_DIM:
            raise ValueError("mean and std: one value or one per channel (12)")
        return t

    @staticmethod
    def _check_count(k: int):
        if k < 1:
            raise ValueError("the class list is empty")
        if k > MAX_CLASSES:
            raise ValueError(f"at most {MAX_CLASSES} classes, got {k}")

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ws(self):
        return self.ws.data_ptr(), self.ws.numel()

    # ------------------------------------------------------------------ API
    def refresh(self):
        """Fold the model's current weights and running statistics into the decoder (after an optimiser step or a
        load_state_dict; until then the decoder keeps the copy of the last fold).  A class table that comes from the model
        (one-hot ids, glove rows) is derived again too, which empties the vote ring.  The adaptive form re-reads weights, gamma
        and beta and keeps its BatchNorm statistics."""
        e = self.engine
        if self.adapt is None:
            _lib.check(self.lib.cp_online_prepare(C.byref(self._cfg), C.byref(e._p), C.byref(e._bn), C.c_float(1e-5), *self._ws(),
                                                  self._stream()), "cp_online_prepare")
        else:
            bn = C.byref(e._bn) if not (e.adabn or self._prepared) else None
            _lib.check(self.lib.cp_online_adapt_prepare(C.byref(self._cfg), C.byref(e._p), bn, C.c_float(1e-5), C.c_double(self.adapt),
                                                        *self._ws(), self._stream()), "cp_online_adapt_prepare")
        self._prepared = True
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
        if sum(x is not None for x in (classes, glove, table)) != 1:
            raise ValueError("set_classes takes exactly one of classes, glove, table")
        e = self.engine
        if glove is not None and e.adabn:
            raise _lib.CpNativeError("glove class rows need a glove encoder with running statistics: on an AdaBN model its "
                                     "batch statistics would come from a zero-padded group; pass classes= or table=")
        if classes is not None:
            cid = torch.as_tensor(np.asarray(classes, dtype=np.int64).reshape(-1))
            self._check_count(cid.numel())
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
            self._check_count(src.shape[0])
            ids_t = torch.arange(src.shape[0]) if ids is None else torch.as_tensor(np.asarray(ids, dtype=np.int64).reshape(-1))
            if ids_t.numel() != src.shape[0]:
                raise ValueError("one id per row")
            rows = src
        if len(set(ids_t.tolist())) != ids_t.numel():
            raise ValueError("class ids must be distinct")
        order = torch.argsort(ids_t)
        ids_t = ids_t[order]
        if rows is None:
            w, b = e.values.views["glove_net.easy.0.weight"], e.values.views["glove_net.easy.0.bias"]
            tab = (w[:, ids_t.to(self.device)].t() + b).contiguous()
        elif glove is not None:
            k = rows.shape[0]
            padded = torch.zeros((k + CP_TASKS - 1) // CP_TASKS * CP_TASKS, 20)     # the glove encoder takes whole groups of 41 rows
            padded[:k] = rows[order]
            zg = e.glove_forward(padded.to(self.device).reshape(1, -1, 20), training=False)
            tab = zg[:k].contiguous()
        else:
            tab = rows[order].to(self.device).contiguous()
        self._source = (classes, glove, table, ids)
        self._table = tab.to(torch.float32).contiguous()
        self.class_ids = ids_t.to(torch.int32)
        self._ids_dev = self.class_ids.to(self.device)
        _lib.check(self.lib.cp_online_set_classes(C.byref(self._cfg), *self._ws(), self._table.data_ptr(), self._ids_dev.data_ptr(),
                                                  int(ids_t.numel()), self._stream()), "cp_online_set_classes")

    def reset(self):
        """Start a new stream: filter, RMS history, sample count and vote ring to zero; classes and weights (and the adaptive
        form's BatchNorm statistics: the same user keeps their calibration) stay."""
        _lib.check(self.lib.cp_online_reset(C.byref(self._cfg), *self._ws(), self._stream()), "cp_online_reset")
        self.n_seen = 0

    def push(self, raw: torch.Tensor, return_logits: bool = False, return_windows: bool = False):
        """raw (n, 12) f32 on the GPU: the next n samples of the stream.  Returns (pred, voted[, logits][, windows]) for the
        M = windows_emitted(n_seen, n, phase) windows the chunk completes: pred, voted (M,) int32 class ids, logits (M, K) f32,
        windows (M, 12) f32 (the normalised windows, a test aid)."""
        if self.class_ids is None:
            raise _lib.CpNativeError("set_classes() first")
        if not self.calibrated:
            raise _lib.CpNativeError("an AdaBN model has no BatchNorm statistics: calibrate() first")
        if raw.device.type != "cuda" or raw.dtype != torch.float32 or raw.dim() != 2 or raw.shape[1] != EMG_DIM:
            raise ValueError("raw must be an (n, 12) float32 tensor on the GPU")
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
            fn = self.lib.cp_online_push if self.adapt is None else self.lib.cp_online_adapt_push
            _lib.check(fn(C.byref(self._cfg), *self._ws(), piece.data_ptr(), n, self.mean_std.data_ptr(),
                          pv[0].data_ptr(), pv[1].data_ptr(), logits.data_ptr() if logits is not None else None,
                          wins.data_ptr() if wins is not None else None, self._stream()), "cp_online_push")
            self.n_seen += n
            outs.append((pred, voted, logits, wins))
        if not outs:
            outs.append((torch.empty(0, dtype=torch.int32, device=self.device),) * 2
                        + (torch.empty(0, K, device=self.device), torch.empty(0, EMG_DIM, device=self.device)))

        def cat(i):
            parts = [o[i] for o in outs]
            return parts[0] if len(parts) == 1 else torch.cat(parts)

        res = [cat(0), cat(1)]
        if return_logits:
            res.append(cat(2))
        if return_windows:
            res.append(cat(3))
        return tuple(res)

    # ------------------------------------------------------------------ adaptive form
    def _need_adapt(self, what: str):
        if self.adapt is None:
            raise _lib.CpNativeError(f"{what} needs the adaptive form: OnlineDecoder(..., adapt=alpha)")

    def calibration_windows(self, raw: torch.Tensor) -> torch.Tensor:
        """The windows a fresh stream would emit for `raw` (n, 12), by the offline path: preprocess_segments + normalize_ with
        this decoder's filter, phase, mean and std."""
        from .preprocess import normalize_, preprocess_segments
        if raw.device.type != "cuda" or raw.dtype != torch.float32 or raw.dim() != 2 or raw.shape[1] != EMG_DIM:
            raise ValueError("raw must be an (n, 12) float32 tensor on the GPU")
        k = windows_before(raw.shape[0], self.phase)
        if k < 2:
            raise ValueError("calibration takes at least 2 windows")
        raw = raw.contiguous()[None]
        keep = self.phase + STRIDE * np.arange(k)
        step = _lib.CP_ONLINE_MAX_WINDOWS                  # positions one call of the offline transform keeps
        w = torch.cat([preprocess_segments(raw, b=self._b, a=self._a, keep=keep[i:i + step]) for i in range(0, k, step)], dim=1)
        return normalize_(w.contiguous(), self.mean_std[0], self.mean_std[1])[0]

    def calibrate(self, raw: torch.Tensor):
        """AdaBN calibration from a recording raw (n, 12) f32 on the GPU: every BatchNorm's statistics become the batch
        statistics of the recording's windows, layer by layer (include/cpnative.h).  Stream state, vote ring and classes stay."""
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
