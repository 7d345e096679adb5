"""CPU-only: the specification of the scaler (include/tdk_hip_resample.h) as a float64 NumPy restatement, pinned to an independent
implementation: torch.nn.functional.interpolate(mode='bilinear', antialias=True, align_corners=False) on the CPU in float64.

Along one axis with n_in source samples and n_out results, for output index i:

    s = n_in / n_out        r = max(s, 1)        c = s (i + 1/2)
    w_j = max(0, 1 - |j + 1/2 - c| / r)     for j in [0, n_in)
    y_i = sum_j w_j x_j / sum_j w_j

and the 2-D result is the horizontal pass followed by the vertical pass.  `resize_ref` shares no code with the product; the GPU
tests (tests/test_gpu_resample.py) load it from this file.  It walks the taps of a window around c instead of building the
n_out x n_in matrix, so a 60 000-wide row or a 12 MP frame stays cheap; samples outside the window have weight 0 by the formula."""
import numpy as np
import pytest
import torch

GEOMETRIES = [  # (h, w) -> (oh, ow)
    ((97, 131), (24, 33)), ((64, 64), (64, 64)), ((300, 400), (75, 100)), ((37, 53), (80, 91)), ((384, 512), (96, 128)),
    ((250, 334), (17, 23)), ((101, 77), (100, 76)), ((50, 60), (1, 1)), ((129, 257), (8, 16)),
    ((64, 1024), (64, 64)), ((1, 17), (1, 5)), ((23, 2), (7, 2)),   # ratio exactly 16 on one axis, a single row, two columns kept
]


def axis_taps(n_in, n_out):
    """(j, w): for every output the source indices of a window that covers its support, and their weights (0 outside the frame
    and outside the triangle), float64."""
    s = n_in / n_out
    r = max(s, 1.0)
    c = s * (np.arange(n_out, dtype=np.float64) + 0.5)
    first = np.floor(c - r).astype(np.int64) - 1
    j = first[:, None] + np.arange(int(np.ceil(2.0 * r)) + 4, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(j + 0.5 - c[:, None]) / r)
    w = np.where((j >= 0) & (j < n_in), w, 0.0)
    return np.clip(j, 0, n_in - 1), w


def filter_axis(x, n_out, axis):
    """One pass along `axis` of a float64 array: sum_j w_j x_j / sum_j w_j."""
    x = np.moveaxis(x, axis, 0)
    j, w = axis_taps(x.shape[0], n_out)
    shape = (n_out,) + (1,) * (x.ndim - 1)
    num = np.zeros((n_out,) + x.shape[1:], np.float64)
    for k in range(j.shape[1]):
        num += w[:, k].reshape(shape) * x[j[:, k]]
    return np.moveaxis(num / w.sum(1).reshape(shape), 0, axis)


def resize_ref(x, out_w, out_h):
    """(H, W, C) -> (out_h, out_w, C) in float64: horizontal pass, then vertical."""
    x = np.asarray(x, dtype=np.float64)
    return filter_axis(filter_axis(x, out_w, 1), out_h, 0)


def max_taps(n_in, n_out):
    """Largest number of samples with a non-zero weight under one output."""
    return int((axis_taps(n_in, n_out)[1] > 0).sum(1).max())


def torch_aa(x, out_w, out_h):
    chw = torch.from_numpy(x).permute(2, 0, 1).unsqueeze(0)
    out = torch.nn.functional.interpolate(chw, size=(out_h, out_w), mode='bilinear', antialias=True, align_corners=False)
    return out.squeeze(0).permute(1, 2, 0).numpy()


@pytest.mark.parametrize('src,dst', GEOMETRIES)
def test_restatement_agrees_with_torch_antialiased_bilinear(src, dst):
    rng = np.random.default_rng(src[0] * 1000 + dst[1])
    x = rng.random((*src, 3))
    mine, theirs = resize_ref(x, dst[1], dst[0]), torch_aa(x, dst[1], dst[0])
    assert mine.shape == theirs.shape == (*dst, 3) and mine.dtype == np.float64
    err = float(np.abs(mine - theirs).max())
    print(f'resize_ref vs torch antialias float64 {src} -> {dst}: {err:.2e}')
    assert err <= 1e-12, (src, dst, err)


def test_upscaling_is_plain_bilinear():
    x = np.random.default_rng(5).random((37, 53, 3))
    chw = torch.from_numpy(x).permute(2, 0, 1).unsqueeze(0)
    plain = torch.nn.functional.interpolate(chw, size=(80, 91), mode='bilinear', align_corners=False).squeeze(0).permute(1, 2, 0).numpy()
    assert np.abs(resize_ref(x, 91, 80) - plain).max() <= 1e-12


def test_identity_has_weight_one_and_tap_counts_stay_within_the_documented_limit():
    x = np.random.default_rng(6).random((9, 11, 1))
    assert np.array_equal(resize_ref(x, 11, 9), x)
    assert max_taps(64, 64) == 1 and max_taps(37, 80) == 2
    for n_in, n_out in ((1024, 64), (65535, 4096), (60000, 4000), (16, 1), (4096, 1024), (4096, 256), (334, 23)):
        assert max_taps(n_in, n_out) <= 32, (n_in, n_out)


def checkerboard(h, w):
    """2 x 2-pixel squares, placed so that the 2 x 2 source pixels plain bilinear reads at 4:1 always lie inside one square."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy + 1) >> 1) + ((xx + 1) >> 1)) & 1).astype(np.float64)[:, :, None]


def test_plain_bilinear_aliases_where_the_specified_filter_does_not():
    """A checkerboard at 4:1: away from the frame's edge the specified filter returns the mean, 1/2; plain bilinear reads only
    squares of one colour and returns 0 everywhere."""
    x = checkerboard(64, 64)
    assert abs(x.mean() - 0.5) < 0.02
    assert np.abs(resize_ref(x, 16, 16)[1:-1, 1:-1] - 0.5).max() <= 1e-15
    chw = torch.from_numpy(x).permute(2, 0, 1).unsqueeze(0)
    plain = torch.nn.functional.interpolate(chw, size=(16, 16), mode='bilinear', align_corners=False)
    assert float(plain.abs().max()) == 0.0
