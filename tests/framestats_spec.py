"""A NumPy restatement of the specification in include/tdk_hip_stats.h: float32 where the header says float32 (one rounding per
written operation), float64 where it says double, Python integers for the counters.  tests/test_framestats_spec.py holds it to
independent evaluations; tests/test_gpu_framestats.py holds the kernels to it, integer for integer and bit for bit."""

import math
from dataclasses import dataclass

import numpy as np

f32 = np.float32
FIXED = 1048576.0   # 2**20: the fixed-point step of `sum` is 1 / FIXED of a bin width
PATTERNS = {'RGGB': 0x94949494, 'BGGR': 0x16161616, 'GRBG': 0x61616161, 'GBRG': 0x49494949}


@dataclass
class Spec:
    hist: np.ndarray          # (C, B) int64
    below: np.ndarray         # (C,) int64 ...
    above: np.ndarray
    nan: np.ndarray
    valid: np.ndarray
    sum: np.ndarray
    mean: np.ndarray          # (C,) float32
    percentiles: np.ndarray   # (C + 1, Q) float32
    gains: np.ndarray         # (3,) float32


def scale_of(bins, lo, hi):
    """(range, scale) as the host computes them."""
    span = f32(f32(hi) - f32(lo))
    return span, f32(f32(bins) / span)


def groups_of(frame, pattern=None, stride=1):
    """(x, channel): x is (groups, members) float32, the sampled groups of one frame in raster order; channel (members,) the channel of
    each member.  frame: (H, W, C) image, or (H, W) mosaic with `pattern` a Bayer pattern word."""
    a = np.asarray(frame)
    if pattern is None:
        assert a.ndim == 3
        x = a[::stride, ::stride].astype(np.float32).reshape(-1, a.shape[2])
        return x, np.arange(a.shape[2])
    assert a.ndim == 2 and a.shape[0] % 2 == 0 and a.shape[1] % 2 == 0
    h, w = a.shape
    cells = a.astype(np.float32).reshape(h // 2, 2, w // 2, 2).transpose(0, 2, 1, 3).reshape(h // 2, w // 2, 4)   # member p = 2 * (i & 1) + (j & 1)
    x = cells[::stride, ::stride].reshape(-1, 4)
    return x, np.array([(pattern >> (2 * p)) & 3 for p in range(4)])


def percentile(hist, q, lo, span, bins):
    """The header's percentile of one histogram (Python integers), q a float32 fraction."""
    n = int(sum(hist))
    if n == 0:
        return f32(lo)
    r = int(min(max(math.ceil(float(f32(q)) * float(n)), 1), n))
    cum = 0
    for b, count in enumerate(hist):
        if cum + int(count) >= r:
            frac = float(r - cum) / float(int(count))
            w = float(span) / float(bins)
            return f32(float(f32(lo)) + (float(b) + frac) * w)
        cum += int(count)
    raise AssertionError('unreachable: cum(B - 1) == N >= r')


def framestats(frames, channels=3, pattern=None, bins=256, value_range=(0.0, 1.0), stride=1, quantiles=(), min_count=64):
    """The statistics of a list of frames pooled into one result."""
    lo, hi = f32(value_range[0]), f32(value_range[1])
    span, scale = scale_of(bins, lo, hi)
    c = 3 if pattern is not None else channels
    hist = np.zeros((c, bins), np.int64)
    below, above, nan, valid, total = (np.zeros(c, np.int64) for _ in range(5))
    for frame in frames:
        x, channel = groups_of(frame, pattern, stride)
        isnan = np.isnan(x)
        with np.errstate(invalid='ignore', over='ignore'):
            t = ((x - lo).astype(np.float32) * scale).astype(np.float32)
            t = np.where(isnan, f32(0), t)   # a NaN never reaches the index conversion
            b = np.minimum(np.maximum(np.floor(t), f32(0)), f32(bins - 1)).astype(np.int64)
            inside = ~isnan & (x >= lo) & (x < hi)
            ok = inside.all(axis=1)
            fixed = np.rint((np.minimum(np.maximum(t, f32(0)), f32(bins)) * f32(FIXED)).astype(np.float32)).astype(np.int64)
        for m, k in enumerate(channel):
            live = ~isnan[:, m]
            hist[k] += np.bincount(b[live, m], minlength=bins)
            below[k] += int(np.count_nonzero(live & (x[:, m] < lo)))
            above[k] += int(np.count_nonzero(live & (x[:, m] >= hi)))
            nan[k] += int(np.count_nonzero(isnan[:, m]))
            valid[k] += int(np.count_nonzero(ok))
            total[k] += int(fixed[ok, m].sum())
    w = float(span) / float(bins)
    mean = np.zeros(c, np.float32)
    for k in range(c):
        if valid[k] >= min_count:
            mean[k] = f32(float(lo) + (float(total[k]) / (float(valid[k]) * FIXED)) * w)
    rows = [hist[k].tolist() for k in range(c)] + [hist.sum(axis=0).tolist()]
    pct = np.array([[percentile(row, q, lo, span, bins) for q in quantiles] for row in rows], np.float32).reshape(c + 1, len(quantiles))
    gains = np.ones(3, np.float32)
    if c == 3 and all(valid[k] >= min_count for k in range(3)) and all(mean[k] > 0 for k in range(3)):
        with np.errstate(over='ignore'):
            gains = np.array([np.minimum(np.maximum(f32(mean[1] / mean[k]), f32(1.0) / f32(64.0)), f32(64.0)) for k in range(3)], np.float32)
    return Spec(hist, below, above, nan, valid, total, mean, pct, gains)
