"""CPU-only: the NumPy restatement of include/tdk_hip_stats.h (tests/framestats_spec.py) held to independent evaluations -- NumPy's own
histograms, float64 means, order statistics -- and to the edge rules the header writes down.  The GPU tests then hold the kernels to
the restatement bit for bit."""

import math

import numpy as np
import pytest

import framestats_spec as spec

f32 = np.float32


def natural(rng, shape, dtype=np.float32):
    """Values that look like a linear frame: most of the range used, a long tail, some out of range on both sides."""
    v = rng.gamma(2.0, 0.12, size=shape) - 0.02
    return v.astype(dtype)


@pytest.mark.parametrize('bins', [2, 64, 256, 1024])
def test_power_of_two_bins_over_the_unit_range_equal_numpy_histogram(bins):
    """With lo = 0, hi = 1 and B a power of two, (x - 0) * B is exact, so floor(t) is the bin NumPy computes in float64 (its last bin is
    closed at 1.0; the header's is open and 1.0 counts as above, landing in the last bin through the clamp all the same)."""
    rng = np.random.default_rng(bins)
    x = rng.random((61, 47, 3), dtype=np.float32)
    x[0, 0] = (0.0, 1.0, np.nextafter(f32(1), f32(0)))
    s = spec.framestats([x], channels=3, bins=bins)
    for k in range(3):
        expected, _ = np.histogram(x[..., k].astype(np.float64), bins=bins, range=(0, 1))
        assert np.array_equal(s.hist[k], expected), k
    assert s.below.tolist() == [0, 0, 0] and s.above.tolist() == [0, 1, 0] and s.nan.tolist() == [0, 0, 0]
    assert s.valid.tolist() == [61 * 47 - 1] * 3   # the pixel whose green is 1.0 is not a valid group


def test_byte_histogram_equals_bincount():
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, size=(53, 39, 1), dtype=np.uint8)
    s = spec.framestats([x], channels=1, bins=256, value_range=(0, 256))
    assert np.array_equal(s.hist[0], np.bincount(x.ravel(), minlength=256))
    assert (s.below[0], s.above[0], s.nan[0], s.valid[0]) == (0, 0, 0, x.size)
    y = rng.integers(0, 65536, size=(40, 30), dtype=np.uint16)   # a 16-bit mosaic into 1024 bins of 64 codes each
    m = spec.framestats([y], pattern=spec.PATTERNS['RGGB'], bins=1024, value_range=(0, 65536))
    assert np.array_equal(m.hist[0], np.bincount(y[0::2, 0::2].ravel() // 64, minlength=1024))
    assert np.array_equal(m.hist[2], np.bincount(y[1::2, 1::2].ravel() // 64, minlength=1024))
    assert np.array_equal(m.hist[1], np.bincount(np.concatenate((y[0::2, 1::2].ravel(), y[1::2, 0::2].ravel())) // 64, minlength=1024))
    assert m.valid.tolist() == [300, 600, 300]


@pytest.mark.parametrize('lo, hi, bins', [(0.0, 1.0, 256), (-0.25, 1.75, 100), (0.0, 4.0, 1024), (-1.0, 1.0, 7)])
def test_mean_is_the_float64_mean_within_the_fixed_point_step(lo, hi, bins):
    """sum / valid is the mean position in bins; every term is off by the three float32 roundings behind t (the difference, the
    scale, the product: each at most 2**-24 of t <= B) and by the fixed point (2**-21), so the mean is within
    (2**-21 + 3 * B * 2**-24) bin widths plus the float32 rounding of the result."""
    rng = np.random.default_rng(bins)
    x = (rng.random((45, 37, 3)) * (hi - lo) * 1.2 + lo - 0.1 * (hi - lo)).astype(np.float32)
    s = spec.framestats([x], channels=3, bins=bins, value_range=(lo, hi), min_count=1)
    ok = ((x >= f32(lo)) & (x < f32(hi))).all(axis=2)
    width = (hi - lo) / bins
    for k in range(3):
        exact = x[..., k][ok].astype(np.float64).mean()
        bound = (2.0 ** -21 + 3 * bins * 2.0 ** -24) * width + 2.0 ** -23 * max(abs(lo), abs(hi))
        print(f'channel {k}: |mean - float64 mean| = {abs(float(s.mean[k]) - exact):.3e}, bound {bound:.3e}')
        assert s.valid[k] == np.count_nonzero(ok)
        assert abs(float(s.mean[k]) - exact) <= bound
        assert abs(s.sum[k] / s.valid[k] / spec.FIXED - (exact - lo) / width) <= 2.0 ** -21 + 3 * bins * 2.0 ** -24


# parameters exactly representable in float32
@pytest.mark.parametrize('lo, hi, bins, stride', [(0.0, 1.0, 256, 1), (0.0, 1.0, 1024, 2), (-0.5, 1.5, 64, 1), (0.0, 2.0, 100, 3), (0.25, 0.75, 17, 1),
                                                  (0.0, 65536.0, 512, 1)])
def test_percentiles_lie_within_one_bin_of_the_order_statistic(lo, hi, bins, stride):
    """The r-th smallest of the values the histogram counted lies in bin b*, and so does the percentile: they differ by less than one
    bin width.  (Values outside the range sit in the edge bins: they are clamped to the range for the comparison.)"""
    rng = np.random.default_rng(bins + stride)
    x = (natural(rng, (90, 70, 3)) * f32(hi - lo) + f32(lo)).astype(np.float32)
    quantiles = (0.0, 0.001, 0.25, 0.5, 0.9, 0.999, 1.0)
    s = spec.framestats([x], channels=3, bins=bins, value_range=(lo, hi), stride=stride, quantiles=quantiles)
    width = (hi - lo) / bins
    sampled = x[::stride, ::stride]
    worst = 0.0
    for row in range(4):
        values = np.sort(np.clip((sampled[..., row] if row < 3 else sampled).astype(np.float64).ravel(), lo, hi))
        for qi, q in enumerate(quantiles):
            r = min(max(math.ceil(float(f32(q)) * values.size), 1), values.size)
            err = abs(float(s.percentiles[row, qi]) - values[r - 1]) / width
            worst = max(worst, err)
            assert err <= 1.0, (row, q, err)
    print(f'lo={lo} hi={hi} bins={bins} stride={stride}: worst |percentile - order statistic| = {worst:.3f} bin widths')


def test_edge_rules():
    lo, hi = f32(0.25), f32(0.75)
    up, down = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    x = np.array([np.nan, np.inf, -np.inf, -0.0, lo, down(lo), up(lo), hi, down(hi), up(hi), 0.5, 0.5], np.float32).reshape(2, 6, 1)
    s = spec.framestats([x], channels=1, bins=8, value_range=(lo, hi), quantiles=(0.0, 1.0), min_count=1)
    assert s.nan[0] == 1 and s.hist.sum() == 11                  # the NaN is in no bin
    assert s.below[0] == 3 and s.above[0] == 3                   # -Inf, -0, lo - ulp;  +Inf, hi (x == hi is above), hi + ulp
    assert s.hist[0, 0] == 3 + 2 and s.hist[0, 7] == 3 + 1       # the clamp puts them into the edge bins, beside lo, lo + ulp and hi - ulp
    assert s.hist[0, 4] == 2 and s.valid[0] == 5                 # 0.5 opens bin 4; valid: lo, lo + ulp, hi - ulp, 0.5, 0.5
    assert s.percentiles[1, 0] > lo and s.percentiles[1, 1] == hi   # q = 0 -> r = 1, inside the first bin; q = 1 -> the top of the last
    # a group with one member out of range (or NaN) contributes to no mean, in any channel
    rgb = np.array([[[0.5, 0.5, 0.5], [0.5, 2.0, 0.5], [0.5, np.nan, 0.5], [0.25, 0.5, 0.75]]], np.float32)
    g = spec.framestats([rgb], channels=3, bins=4, value_range=(0, 1), min_count=1)
    assert g.valid.tolist() == [2, 2, 2] and g.nan.tolist() == [0, 1, 0] and g.above.tolist() == [0, 1, 0]
    assert g.hist.sum(axis=1).tolist() == [4, 3, 4]
    assert g.mean.tolist() == [0.375, 0.5, 0.625]
    assert g.gains.tolist() == [float(f32(0.5) / f32(0.375)), 1.0, float(f32(0.5) / f32(0.625))]


def test_empty_histogram_min_count_and_the_gain_clamp():
    nothing = np.full((4, 4, 3), np.nan, np.float32)
    s = spec.framestats([nothing], channels=3, bins=16, value_range=(-2, 2), quantiles=(0.0, 0.5, 1.0))
    assert s.hist.sum() == 0 and s.nan.tolist() == [16] * 3
    assert (s.percentiles == f32(-2)).all() and (s.mean == 0).all() and s.gains.tolist() == [1, 1, 1]
    # every value out of range: N > 0, valid = 0 -- percentiles come from the edge bins, no mean, no gains
    out = np.full((4, 4, 3), 9.0, np.float32)
    s = spec.framestats([out], channels=3, bins=16, value_range=(0, 1), quantiles=(0.5,), min_count=1)
    assert s.hist[:, 15].tolist() == [16] * 3 and s.valid.tolist() == [0] * 3 and s.above.tolist() == [16] * 3
    assert (s.mean == 0).all() and s.gains.tolist() == [1, 1, 1]
    assert s.percentiles[3, 0] == f32(15.5 / 16)                       # r = 24 of 48 in the last bin
    # min_count: 15 valid pixels are not enough for 16
    x = np.full((4, 4, 3), (0.2, 0.4, 0.1), np.float32)
    x[0, 0, 2] = np.nan
    assert spec.framestats([x], bins=16, min_count=16).gains.tolist() == [1, 1, 1]
    few = spec.framestats([x], bins=16, min_count=15)
    assert few.gains[1] == 1 and few.gains[0] == f32(few.mean[1] / few.mean[0]) and abs(few.gains[2] - 4) < 1e-5
    # the clamp: a channel 1000 times darker than green gets 64, one 1000 times brighter 1/64
    y = np.full((8, 8, 3), (0.0005, 0.5, 500.0), np.float32)
    clamped = spec.framestats([y], bins=1024, value_range=(0, 1024), min_count=1)
    assert clamped.gains.tolist() == [64.0, 1.0, 1.0 / 64.0]
    # a mean of zero (every valid value at lo) switches the gains off
    z = np.zeros((8, 8, 3), np.float32)
    assert spec.framestats([z], bins=8, min_count=1).gains.tolist() == [1, 1, 1]
    # one channel: no gains
    assert spec.framestats([z[..., :1]], channels=1, bins=8, min_count=1).gains.tolist() == [1, 1, 1]


def test_mosaic_cells_stride_and_sets():
    rng = np.random.default_rng(3)
    m = rng.random((12, 20), dtype=np.float32)
    for name, word in spec.PATTERNS.items():
        s = spec.framestats([m], pattern=word, bins=32, stride=1, min_count=1)
        planes = {p: m[p // 2::2, p % 2::2] for p in range(4)}
        for k in range(3):
            members = np.concatenate([planes[p].ravel() for p in range(4) if (word >> (2 * p)) & 3 == k])
            assert np.array_equal(s.hist[k], np.histogram(members.astype(np.float64), bins=32, range=(0, 1))[0]), (name, k)
        assert s.valid.tolist() == [60, 120, 60]
    # stride 3 on cells: cell rows 0 and 3, cell columns 0, 3, 6, 9
    s = spec.framestats([m], pattern=spec.PATTERNS['RGGB'], bins=32, stride=3, min_count=1)
    assert s.hist.sum(axis=1).tolist() == [8, 16, 8]
    reds = m[0::2, 0::2][::3, ::3]
    assert np.array_equal(s.hist[0], np.histogram(reds.astype(np.float64), bins=32, range=(0, 1))[0])
    # a stride beyond the frame keeps the first group only
    assert spec.framestats([m], pattern=spec.PATTERNS['RGGB'], bins=32, stride=50).hist.sum(axis=1).tolist() == [1, 2, 1]
    # a set pools: the counters add, the derived values are those of the concatenation
    a, b, c = (rng.random((9, 11, 3), dtype=np.float32) for _ in range(3))
    q = (0.01, 0.5, 0.99)
    pooled = spec.framestats([a, b, c], bins=64, quantiles=q, min_count=1)
    joined = spec.framestats([np.concatenate((a, b, c), axis=0)], bins=64, quantiles=q, min_count=1)
    for field in ('hist', 'below', 'above', 'nan', 'valid', 'sum', 'mean', 'percentiles', 'gains'):
        assert np.array_equal(getattr(pooled, field), getattr(joined, field)), field
