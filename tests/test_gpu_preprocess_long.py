"""cp_preprocess_emg on segments longer than 32,767 and 65,535 samples (a whole recording as one segment, as
`_calibration_windows` passes it): kept positions on both sides of the two places where a 16-bit position would wrap,
bit for bit against the numpy oracle, for the <9 coefficients, window 11> kernel and the general one."""
import numpy as np
import pytest
import torch

from oracle import preprocess_cpu as pp

pytestmark = pytest.mark.gpu

S, L = 2, 66100                  # the smallest round length with kept positions on both sides of 32,768 and of 65,536
GAIN = np.float32(1024)


def _rms_series(raw, b, a, win):
    """the whole RMS series of raw (S, L, 12) by the oracle, both segments at once: (S, L - 2 (win // 2), 12) float32"""
    half = win // 2
    x = np.ascontiguousarray(raw.transpose(1, 0, 2))                         # the oracle runs along axis 0
    y = pp.lfilter_df2t(b, a, x * GAIN).astype(np.float32)
    r = np.sqrt(pp.uniform_filter1d_nearest(np.square(y), win))[half:x.shape[0] - half]
    return np.ascontiguousarray(r.transpose(1, 0, 2))


@pytest.fixture(scope="module")
def raw():
    """seeded noise at the amplitude of test_oracle_preprocess.raw_segments; the second segment at another scale, so that
    a wrong segment offset s * L * 12 cannot pass"""
    rng = np.random.default_rng(66100)
    x = 2e-5 * rng.standard_normal((S, L, 12))
    x[1] *= 1.7
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def dev_raw(raw):
    return torch.from_numpy(raw).cuda()


@pytest.fixture(scope="module")
def full(raw):
    b, a = pp.butter_bandpass()
    out = _rms_series(raw, b, a, 11)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def full_generic(raw):
    b, a = pp.butter_bandpass(order=2, low_hz=30.0, high_hz=400.0)
    out = _rms_series(raw, b, a, 7)
    out.setflags(write=False)
    return out


def _check(dev_raw, ref, keep, **kw):
    from contrastiveprosthetics_amd import preprocess as P
    keep = np.asarray(keep)
    got = P.preprocess_segments(dev_raw, keep=keep, **kw).cpu().numpy()      # the wrapper's output starts as torch.empty
    assert got.shape == (dev_raw.shape[0], len(keep), 12)
    bad = np.flatnonzero(~np.isfinite(got).all(axis=(0, 2)))
    assert np.isfinite(got).all(), f"slots never written or not finite: {bad.tolist()} (positions {keep[bad].tolist()})"
    want = ref[:, keep]
    diff = np.flatnonzero((got != want).any(axis=(0, 2)))
    print(f"{len(keep)} kept positions {int(keep.min())}..{int(keep.max())}: {diff.size} slots differ from the oracle")
    assert np.array_equal(got, want), f"slots {diff.tolist()} (positions {keep[diff].tolist()}) differ from the oracle"


def test_positions_across_both_wrap_points(dev_raw, full):
    b, a = pp.butter_bandpass()
    n_rms = L - 10
    assert full.shape == (S, n_rms, 12) and n_rms - 1 == 66089
    # unsorted, with repeats, on both sides of 32,768 and 65,536, and both ends of the series
    keep = np.concatenate(([0], np.arange(32760, 32776), np.arange(65528, 65544), [n_rms - 1, 32768, 5]))
    assert {32767, 32768, 65535, 65536} <= set(keep.tolist())
    _check(dev_raw, full, keep, b=b, a=a)
    # wholly above 65,536: every 16-bit copy of these positions is a small positive number
    _check(dev_raw, full, np.arange(65540, n_rms, 7)[:70], b=b, a=a)
    # 256 positions 20 apart from 32,000: a chunk of _calibration_windows that straddles 32,768
    keep = 32000 + 20 * np.arange(256)
    assert keep[0] < 32768 < keep[-1] < 65536
    _check(dev_raw, full, keep, b=b, a=a)


def test_generic_kernel_long(dev_raw, full_generic):
    """another filter order and window: the general kernel, reference built as in
    test_gpu_preprocess.test_other_filter_orders_and_windows_generic_kernel"""
    b, a = pp.butter_bandpass(order=2, low_hz=30.0, high_hz=400.0)
    n_rms = L - 6
    assert full_generic.shape == (S, n_rms, 12)
    keep = np.concatenate((np.arange(32764, 32772), [n_rms - 1], np.arange(65532, 65540), [3, 65536]))
    _check(dev_raw[:1].contiguous(), full_generic[:1], keep, b=b, a=a, rms_window=7)
    _check(dev_raw, full_generic, keep, b=b, a=a, rms_window=7)              # and with the second segment's offset


def test_last_position_is_kept_and_the_next_refused(dev_raw, full):
    from contrastiveprosthetics_amd import preprocess as P
    b, a = pp.butter_bandpass()
    n_rms = L - 10
    with pytest.raises(Exception):
        P.preprocess_segments(dev_raw, b, a, keep=[n_rms])                   # outside the RMS series
    _check(dev_raw, full, [n_rms - 1], b=b, a=a)
