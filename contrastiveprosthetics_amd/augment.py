"""sEMG augmentation of the group gather (include/cpnative.h, cp_gather_groups_aug): what a re-donned sleeve, a
drifting contact and a dead electrode do to the 12 channels of a window, applied in the launch that writes the encoder's
input.  An extension of the data path with no counterpart in the reference, off unless an ``Augment`` is handed over:

    aug = Augment(shift=(-1, 1), gain_sigma=0.35, seed=7)
    dataset.augment = aug                      # TaskWrapper.batch, train mode
    dataset.perturb = Augment(shift=2)         # TaskWrapper.batch, val / test mode: a sleeve turned by two electrodes

``Augment`` owns the stream of draws: ``count`` is the number of gathers drawn so far, and gather k uses the salt
``(k * 0x9E3779B1) & 0xFFFFFFFF``.  ``Augment.reference`` is the definition of what the kernel computes, in numpy: the
integer draws exactly, the arithmetic behind them in float64.
"""
from __future__ import annotations

import numpy as np

from . import _lib

EMG_DIM, RING = 12, 8
NORM_C = np.float32(1.0 / np.sqrt((65536.0 ** 2 - 1.0) / 3.0))       # unit variance of the sum of four 16-bit draws
_M = np.uint64(0xFFFFFFFF)


def salt_of(k: int) -> int:
    """The salt of the k-th gather of a stream (k = 1 for the first)."""
    return (int(k) * 0x9E3779B1) & 0xFFFFFFFF


def hash32(x) -> np.ndarray:
    """hash32 of csrc/common.cuh on uint32 values (carried in uint64, reduced mod 2^32 after every step)."""
    x = np.asarray(x, dtype=np.uint64) & _M
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M
    x = x ^ (x >> np.uint64(16))
    return x


def _words(k: np.ndarray, j) -> np.ndarray:
    """word(j) = h(k ^ (j * 0x85EBCA6B + 0xC2B2AE35)); k (...,) and j broadcast."""
    j = np.asarray(j, dtype=np.uint64)
    return hash32(k ^ ((j * np.uint64(0x85EBCA6B) + np.uint64(0xC2B2AE35)) & _M))


def _normal(k: np.ndarray, j) -> np.ndarray:
    """Irwin-Hall normal from the four 16-bit halves of word(j) and word(j + 1): f32, as the kernel forms it."""
    a, b = _words(k, j), _words(k, np.asarray(j, dtype=np.uint64) + np.uint64(1))
    s = ((a & np.uint64(0xFFFF)) + (a >> np.uint64(16)) + (b & np.uint64(0xFFFF)) + (b >> np.uint64(16))).astype(np.int64) - 131070
    return s.astype(np.float32) * NORM_C


class Augment:
    """shift: a fixed ring shift s, or (lo, hi) for a uniform draw per item, -7 <= lo <= hi <= 7 (model channel d < 8 reads
    source channel (d + s) mod 8: ``online.rotations()[s % 8]``).  p_drop: probability that a channel is dead for an item;
    dead: channels that always are; a dead channel stores `fill`.  gain_sigma / amp_sigma: log-normal gain per (item, channel)
    / per item, on the raw RMS value when mean_std -- 24 floats, [d] mean and [12 + d] std, the online decoders' layout -- is
    given, else on the normalised value.  noise_sigma: additive noise per element, normalised units.  All off by default."""

    def __init__(self, shift=0, p_drop: float = 0.0, dead=(), gain_sigma: float = 0.0, amp_sigma: float = 0.0,
                 noise_sigma: float = 0.0, fill: float = 0.0, mean_std=None, seed: int = 0):
        try:
            lo, hi = (int(shift), int(shift)) if np.isscalar(shift) else (int(shift[0]), int(shift[1]))
            if not np.isscalar(shift) and len(shift) != 2:
                raise TypeError
        except (TypeError, IndexError):
            raise ValueError("shift: an integer or a (lo, hi) pair") from None
        if not (-7 <= lo <= hi <= 7):
            raise ValueError("shift: -7 <= lo <= hi <= 7")
        if not (0.0 <= float(p_drop) <= 1.0):                        # (NaN fails)
            raise ValueError("p_drop must lie in [0, 1]")
        for name, v in (("gain_sigma", gain_sigma), ("amp_sigma", amp_sigma), ("noise_sigma", noise_sigma)):
            if not (0.0 <= float(v) <= 2.0):
                raise ValueError(f"{name} must be finite and lie in [0, 2]")
        if not np.isfinite(float(fill)):
            raise ValueError("fill must be finite")
        dead = tuple(int(d) for d in dead)
        if any(d < 0 or d >= EMG_DIM for d in dead):
            raise ValueError(f"dead: channels in 0..{EMG_DIM - 1}")
        if mean_std is not None:
            mean_std = np.ascontiguousarray(np.asarray(mean_std, dtype=np.float32).reshape(-1))
            if mean_std.shape[0] != 2 * EMG_DIM or not np.isfinite(mean_std).all() or (mean_std[EMG_DIM:] <= 0).any():
                raise ValueError("mean_std: 24 finite floats, [d] mean and [12 + d] std > 0")
        if not (0 <= int(seed) < 2 ** 32):
            raise ValueError("seed: 0 .. 2^32 - 1")
        self.shift = (lo, hi)
        # the settings as the C side holds them (float): the numpy restatement must start from the same values
        self.p_drop, self.gain_sigma, self.amp_sigma, self.noise_sigma, self.fill = (
            float(np.float32(v)) for v in (p_drop, gain_sigma, amp_sigma, noise_sigma, fill))
        self.dead = tuple(sorted(set(dead)))
        self.dead_mask = sum(1 << d for d in self.dead)
        self.mean_std = mean_std
        self.seed = int(seed)
        self.count = 0                          # gathers drawn so far
        self._ms_dev = {}

    @property
    def active(self) -> bool:
        return bool(self.shift != (0, 0) or self.p_drop > 0 or self.dead_mask or self.gain_sigma > 0 or self.amp_sigma > 0
                    or self.noise_sigma > 0)

    def config(self) -> dict:
        return dict(shift=self.shift, p_drop=self.p_drop, dead=self.dead, gain_sigma=self.gain_sigma, amp_sigma=self.amp_sigma,
                    noise_sigma=self.noise_sigma, fill=self.fill,
                    mean_std=None if self.mean_std is None else self.mean_std.copy(), seed=self.seed)

    @property
    def drop_thresh(self) -> int:
        return int(np.floor(self.p_drop * 65536.0 + 0.5))

    def next_salt(self) -> int:
        """Advance the stream by one gather and return its salt."""
        self.count += 1
        return salt_of(self.count)

    def struct(self, salt: int, item_offset: int = 0, device=None, state_addr: int = 0) -> "_lib.cp_augment":
        """The cp_augment of one launch.  state_addr: device address of a cp_step_state whose aug_salt word holds the salt
        (graph replay), else `salt` is used."""
        a = _lib.cp_augment()
        a.seed, a.salt = self.seed, int(salt) & 0xFFFFFFFF
        a.salt_state_lo, a.salt_state_hi = state_addr & 0xFFFFFFFF, state_addr >> 32
        a.shift_min, a.shift_max = self.shift
        a.dead_mask = self.dead_mask
        a.p_drop, a.gain_sigma, a.amp_sigma, a.noise_sigma, a.fill = (self.p_drop, self.gain_sigma, self.amp_sigma,
                                                                      self.noise_sigma, self.fill)
        a.item_offset = int(item_offset)
        if self.mean_std is not None:
            import torch
            key = str(device)
            if key not in self._ms_dev:
                self._ms_dev[key] = torch.from_numpy(self.mean_std).to(device)
            a.mean_std = self._ms_dev[key].data_ptr()
        return a

    # ------------------------------------------------------------------ the definition (numpy)
    def draws(self, item0: int, n_items: int, V: int, salt: int) -> dict:
        """The draws of items item0 .. item0 + n_items - 1 under `salt`, as the kernel forms them: shift (n,) int64 in
        shift_min..shift_max, dead (n, 12) bool (p_drop and `dead` together), n_gain (n, 12), n_amp (n,) and n_noise (n, V, 12)
        f32 normals (bit for bit the kernel's).  A setting that is off leaves zeros."""
        items = (np.arange(n_items, dtype=np.uint64) + np.uint64(int(item0))) & _M
        k0 = hash32(np.uint64(self.seed) ^ hash32(np.uint64((int(salt) + 0x9E3779B9) & 0xFFFFFFFF)))
        k = hash32((k0 + items) & _M)
        lo, hi = self.shift
        shift = np.full(n_items, lo, dtype=np.int64)
        if hi > lo:
            shift = lo + ((_words(k, 0) * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)
        dead = np.zeros((n_items, EMG_DIM), dtype=bool)
        if self.drop_thresh:
            d = np.arange(EMG_DIM, dtype=np.uint64)
            w = _words(k[:, None], np.uint64(1) + d[None, :] // np.uint64(2))
            half = (w >> (np.uint64(16) * (d[None, :] & np.uint64(1)))) & np.uint64(0xFFFF)
            dead = half < np.uint64(self.drop_thresh)
        for d in self.dead:
            dead[:, d] = True
        n_gain = np.zeros((n_items, EMG_DIM), dtype=np.float32)
        if self.gain_sigma > 0:
            n_gain = _normal(k[:, None], 8 + 2 * np.arange(EMG_DIM)[None, :])
        n_amp = _normal(k, 32) if self.amp_sigma > 0 else np.zeros(n_items, dtype=np.float32)
        n_noise = np.zeros((n_items, V, EMG_DIM), dtype=np.float32)
        if self.noise_sigma > 0:
            e = 12 * np.arange(V)[:, None] + np.arange(EMG_DIM)[None, :]
            n_noise = _normal(k[:, None, None], 34 + 2 * e[None])
        return dict(shift=shift, dead=dead, n_gain=n_gain, n_amp=n_amp, n_noise=n_noise)

    def reference(self, x_rows, item0: int, V: int, salt: int, parts: bool = False):
        """What cp_gather_groups_aug stores for the plain gather's rows x_rows (rows, 12): row r belongs to item
        item0 + r // V and is its sample r % V.  float64 (rows, 12).  parts=True also returns, per element, the source channel
        c, the gain G, the noise term and the dead flag (what an error bound is made of)."""
        x = np.asarray(x_rows, dtype=np.float32).reshape(-1, EMG_DIM).astype(np.float64)
        rows = x.shape[0]
        n_items = (rows + V - 1) // V
        dr = self.draws(item0, n_items, V, salt)
        it, v = np.arange(rows) // V, np.arange(rows) % V
        d = np.arange(EMG_DIM)
        s = dr["shift"][it][:, None] % RING
        c = np.where(d[None, :] < RING, (d[None, :] + s) % RING, d[None, :])
        xc = np.take_along_axis(x, c, axis=1)
        G = (np.exp(self.gain_sigma * dr["n_gain"].astype(np.float64))[it]
             * np.exp(self.amp_sigma * dr["n_amp"].astype(np.float64))[it][:, None])
        if self.mean_std is not None:
            mean, std = self.mean_std[:EMG_DIM].astype(np.float64), self.mean_std[EMG_DIM:].astype(np.float64)
            y = ((xc * std[c] + mean[c]) * G - mean[None, :]) / std[None, :]
            y = np.where((c == d[None, :]) & (G == 1.0), x, y)
        else:
            y = xc * G
        noise = self.noise_sigma * dr["n_noise"].astype(np.float64)[it, v]
        y = y + noise
        dead = dr["dead"][it]
        y = np.where(dead, self.fill, y)
        if parts:
            return y, dict(c=c, G=G, noise=noise, dead=dead, shift=dr["shift"][it])
        return y
