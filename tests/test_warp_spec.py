"""CPU-only: the specification of the warp (head comment of include/tdk_hip_warp.h) as two NumPy restatements -- `warp_ref` in
float32 with the exact operation order (what the kernel must reproduce bit for bit; NumPy rounds every float32 operation once and
never contracts), and the same code in float64, pinned here to an independent implementation: torch.nn.functional.grid_sample on
the CPU in float64, align_corners=True, with the grid built from the float64 sx, sy.

    u = (float)j;  v = (float)i
    X = (h0*u + h1*v) + h2;   Y = (h3*u + h4*v) + h5;   Z = (h6*u + h7*v) + h8
    iz = 1 / Z;  x = X*iz;  y = Y*iz
    x2 = x*x;  y2 = y*y;  r2 = x2 + y2;  xy = x*y
    rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1
    tx = p1*(xy + xy) + p2*(r2 + (x2 + x2));   ty = p1*(r2 + (y2 + y2)) + p2*(xy + xy)
    xd = x*rad + tx;   yd = y*rad + ty;   sx = fx*xd + cx;   sy = fy*yd + cy

The restatements share no code with the product; the GPU tests (tests/test_gpu_warp.py) load them from this file."""
import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64


def homography_map(H):
    return [*np.asarray(H, dtype=F64).reshape(-1), 1, 1, 0, 0, 0, 0, 0, 0, 0]


def undistort_map(K, dist, Knew=None, R=None):
    """h = inv(Knew @ R) in float64; dist = (k1, k2, p1, p2, k3)."""
    K = np.asarray(K, dtype=F64)
    Knew = K if Knew is None else np.asarray(Knew, dtype=F64)
    R = np.eye(3) if R is None else np.asarray(R, dtype=F64)
    return [*np.linalg.inv(Knew @ R).reshape(-1), K[0, 0], K[1, 1], K[0, 2], K[1, 2], *dist]


def coords_ref(m, dw, dh, dtype=F32, parts=False):
    """(sx, sy, outside) before the clamp, each (dh, dw).  The map is rounded to float32 first: it is 18 floats in either
    restatement.  parts=True also returns (fx*xd, fy*yd), the magnitudes the rounding bound of the coordinates speaks of."""
    m = np.asarray(m, dtype=F64).astype(F32).astype(dtype)
    one = dtype(1)
    u, v = np.arange(dw, dtype=dtype)[None, :], np.arange(dh, dtype=dtype)[:, None]
    with np.errstate(all='ignore'):
        X = (m[0] * u + m[1] * v) + m[2]
        Y = (m[3] * u + m[4] * v) + m[5]
        Z = (m[6] * u + m[7] * v) + m[8]
        iz = one / Z
        x, y = X * iz, Y * iz
        x2, y2 = x * x, y * y
        r2, xy = x2 + y2, x * y
        rad = ((m[17] * r2 + m[14]) * r2 + m[13]) * r2 + one
        tx = m[15] * (xy + xy) + m[16] * (r2 + (x2 + x2))
        ty = m[15] * (r2 + (y2 + y2)) + m[16] * (xy + xy)
        xd, yd = x * rad + tx, y * rad + ty
        fxd, fyd = m[9] * xd, m[10] * yd
        sx, sy = fxd + m[11], fyd + m[12]
    assert sx.dtype == dtype and sy.dtype == dtype
    outside = ~(Z > 0) | ~np.isfinite(sx) | ~np.isfinite(sy)
    return (sx, sy, outside, fxd, fyd) if parts else (sx, sy, outside)


def c1(t):
    k = t.dtype.type
    return ((k(1.25) * t - k(2.25)) * t) * t + k(1)


def c2(t):
    k = t.dtype.type
    return ((k(-0.75) * t + k(3.75)) * t - k(6)) * t + k(3)


def weights_ref(a, interp):
    """[(tap offset, weight)] for the fraction array a."""
    one = a.dtype.type(1)
    if interp == 'bilinear':
        return [(0, one - a), (1, a)]
    return [(-1, c2(a + one)), (0, c1(a)), (1, c1(one - a)), (2, c2((one + one) - a))]


def split_ref(s, n):
    k = s.dtype.type
    s = np.minimum(np.maximum(s, k(-4)), k(n + 3))
    s0 = np.floor(s)
    return s0.astype(np.int64), s - s0


def store_ref(y, storage):
    """The rounding at the store: float32 as it is, binary16 to nearest even, uint8 rint() after clamping to [0, 255]."""
    if storage == np.uint8:
        return np.rint(np.minimum(np.maximum(y, y.dtype.type(0)), y.dtype.type(255))).astype(np.uint8)
    return y.astype(storage)


def warp_ref(img, m, out_size, interp='bicubic', border='constant', fill=0.0, dtype=F32, store=True):
    """img: (H, W, C) float32, float16 or uint8 -> (dh, dw, C).  dtype=float32, store=True: the bits the kernel must give, in
    the storage type of img.  store=False returns the unrounded result in `dtype`."""
    sh, sw, C = img.shape
    dw, dh = out_size
    src = img.astype(dtype)   # exact for all three storage types
    fill = dtype(fill)
    sx, sy, outside = coords_ref(m, dw, dh, dtype)
    sx, sy = np.where(outside, dtype(0), sx), np.where(outside, dtype(0), sy)
    ix, ax = split_ref(sx, sw)
    iy, ay = split_ref(sy, sh)
    wx, wy = weights_ref(ax, interp), weights_ref(ay, interp)
    acc = None
    for oy, w_y in wy:
        y = iy + oy
        row = None
        for ox, w_x in wx:
            x = ix + ox
            s = src[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)]   # (dh, dw, C)
            if border == 'constant':
                s = np.where(((x >= 0) & (x < sw) & (y >= 0) & (y < sh))[:, :, None], s, fill)
            term = s * w_x[:, :, None]
            row = term if row is None else row + term
        term = row * w_y[:, :, None]
        acc = term if acc is None else acc + term
    out = np.where(outside[:, :, None], fill, acc)
    assert out.dtype == dtype
    return store_ref(out, img.dtype.type) if store else out


# ---------------------------------------------------------------- the maps the CPU and GPU tests share

def rotation_perspective_distortion_map(src_size, dst_size, angle_deg=20.0, f_scale=1.0, persp=(6e-4, -4e-4)):
    """A camera with distortion looking at a rotated, slightly tilted output plane: some output pixels land outside the source."""
    sw, sh = src_size
    dw, dh = dst_size
    f = f_scale * sw
    K = [[f, 0, (sw - 1) / 2], [0, f * 1.02, (sh - 1) / 2], [0, 0, 1]]
    a = np.deg2rad(angle_deg)
    cu, cv = (dw - 1) / 2, (dh - 1) / 2
    to_centre = np.array([[1, 0, -cu], [0, 1, -cv], [0, 0, 1]], dtype=F64)
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [persp[0], persp[1], 1]], dtype=F64)
    scale = np.diag([1.25 * sw / dw / f, 1.25 * sw / dw / f, 1.0])   # the output covers a quarter more than the source sees
    h = scale @ rot @ to_centre
    return [*h.reshape(-1), K[0][0], K[1][1], K[0][2], K[1][2], -0.12, 0.09, 8e-4, -5e-4, -0.02]


def camera_map(size, out_size=None, zoom=1.0):
    """The undistort map of the 4096 x 3000 camera of the issue (f = 2950), scaled to the frame; with out_size a new camera
    matrix that shows the same field of view (times 1 / zoom) at that size."""
    w, h = size
    s = w / 4096.0
    K = [[2950.0 * s, 0, 2040.3 * s], [0, 2946.0 * s, 1507.7 * s * (h / (3000.0 * s))], [0, 0, 1]]
    dist = (-0.12, 0.09, 8e-4, -5e-4, -0.02)
    if out_size is None:
        return undistort_map(K, dist)
    ow, oh = out_size
    t = zoom * ow / w
    Knew = [[K[0][0] * t, 0, (ow - 1) / 2], [0, K[1][1] * t, (oh - 1) / 2], [0, 0, 1]]
    return undistort_map(K, dist, Knew)


def grid_sample_f64(img, sx, sy, interp, border):
    sh, sw, _ = img.shape
    grid = np.stack([2.0 * sx / (sw - 1) - 1.0, 2.0 * sy / (sh - 1) - 1.0], axis=-1)[None]
    chw = torch.from_numpy(img.astype(F64)).permute(2, 0, 1).unsqueeze(0)
    out = torch.nn.functional.grid_sample(chw, torch.from_numpy(grid), mode=interp, padding_mode={'constant': 'zeros', 'replicate': 'border'}[border],
                                          align_corners=True)
    return out.squeeze(0).permute(1, 2, 0).numpy()


SPEC_SRC, SPEC_DST = (61, 47), (53, 41)   # (width, height)


@pytest.mark.parametrize('interp', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('border', ['constant', 'replicate'])
def test_float64_restatement_agrees_with_grid_sample(interp, border):
    m = rotation_perspective_distortion_map(SPEC_SRC, SPEC_DST)
    img = np.random.default_rng(11).random((SPEC_SRC[1], SPEC_SRC[0], 3))
    sx, sy, outside = coords_ref(m, *SPEC_DST, dtype=F64)
    assert not outside.any()   # Z > 0 everywhere: grid_sample has no notion of an outside pixel
    inside = (sx >= 0) & (sx <= SPEC_SRC[0] - 1) & (sy >= 0) & (sy <= SPEC_SRC[1] - 1)
    assert 0.6 <= inside.mean() <= 0.8, inside.mean()   # some taps fall outside, most pixels inside
    mine = warp_ref(img, m, SPEC_DST, interp, border, 0.0, dtype=F64, store=False)
    theirs = grid_sample_f64(img, sx, sy, interp, border)
    assert mine.shape == theirs.shape == (SPEC_DST[1], SPEC_DST[0], 3) and mine.dtype == F64
    err = float(np.abs(mine - theirs).max())
    print(f'warp_ref float64 vs grid_sample {interp}/{border}: {err:.2e}, {inside.mean():.2f} of the pixels inside')
    assert err <= 1e-12, (interp, border, err)


def test_float32_coordinates_stay_within_the_rounding_count():
    """At most 12 roundings on the way to sx, each relative 2^-24 of a magnitude no larger than M = max(|sx|, |fx xd|, |cx|):
    |sx32 - sx64| <= 12 * 2^-24 * M, likewise sy.  (4096 x 3000, f = 2950: the bound is 2.9e-3 px.)"""
    m = camera_map((4096, 3000))
    m32 = np.asarray(m, dtype=F32)
    sx32, sy32, out32 = coords_ref(m, 4096, 3000, F32)
    sx64, sy64, out64, fxd, fyd = coords_ref(m, 4096, 3000, F64, parts=True)
    assert not out32.any() and not out64.any()
    for name, s32, s64, prod, c in (('sx', sx32, sx64, fxd, m32[11]), ('sy', sy32, sy64, fyd, m32[12])):
        M = np.maximum(np.maximum(np.abs(s64), np.abs(prod)), abs(float(c)))
        bound = 12 * 2.0 ** -24 * M
        err = np.abs(s32.astype(F64) - s64)
        print(f'{name}: float32 against float64 at most {err.max():.2e} px, bound at most {bound.max():.2e} px, worst ratio {(err / bound).max():.3f}')
        assert (err <= bound).all(), (name, float((err / bound).max()))
        assert bound.max() < 3.5e-3


def test_identity_map_returns_the_pixel_grid_and_the_input():
    m = homography_map(np.eye(3))
    sx, sy, outside = coords_ref(m, 300, 200)
    assert sx.dtype == F32 and not outside.any()
    assert np.array_equal(sx, np.broadcast_to(np.arange(300, dtype=F32)[None, :], (200, 300)))
    assert np.array_equal(sy, np.broadcast_to(np.arange(200, dtype=F32)[:, None], (200, 300)))
    rng = np.random.default_rng(3)
    for img in (rng.random((29, 37, 3)).astype(F32), rng.random((29, 37, 1)).astype(np.float16), rng.integers(0, 256, (29, 37, 3), dtype=np.uint8)):
        for interp in ('bilinear', 'bicubic'):
            for border in ('constant', 'replicate'):
                out = warp_ref(img, m, (37, 29), interp, border, 9.0)
                assert out.dtype == img.dtype and np.array_equal(out, img), (img.dtype, interp, border)


def test_weights_at_zero_fraction_are_exactly_0_1_0_0():
    zero = np.zeros(1, dtype=F32)
    assert [float(w[0]) for _, w in weights_ref(zero, 'bicubic')] == [0.0, 1.0, 0.0, 0.0]
    assert [float(w[0]) for _, w in weights_ref(zero, 'bilinear')] == [1.0, 0.0]
    assert [o for o, _ in weights_ref(zero, 'bicubic')] == [-1, 0, 1, 2] and [o for o, _ in weights_ref(zero, 'bilinear')] == [0, 1]
    # the Keys kernel with A = -0.75: a partition of unity and symmetric, to rounding -- a weight is six float64 operations on
    # magnitudes of at most 6, so 6 * 6 * 2^-53 = 4e-15 each and 1.6e-14 for the sum of four
    a = np.linspace(0, 1, 1001).astype(F64)
    w = [w for _, w in weights_ref(a, 'bicubic')]
    assert np.abs(sum(w) - 1).max() <= 1.6e-14
    assert np.abs(w[0] - w[3][::-1]).max() <= 8e-15 and np.abs(w[1] - w[2][::-1]).max() <= 8e-15


def test_from_transform_equals_pipeline_transform_through_the_restatement(td):
    from torch_darktable.pipeline.transform import ImageTransform, transform, transformed_size

    cuda = torch.device('cuda', 0)   # a device object only: nothing below reaches the GPU
    w, h = 53, 41
    ramp = (np.arange(h * w * 3, dtype=np.int64).reshape(h, w, 3) % 251).astype(np.uint8)
    for t in ImageTransform:
        wp = td.Warp.from_transform(cuda, (w, h), t)
        m = wp.map
        assert wp.output_size == transformed_size((w, h), t) and np.array_equal(m, np.rint(m)), t
        want = transform(torch.from_numpy(ramp), t).numpy()
        for interp in ('bilinear', 'bicubic'):
            got = warp_ref(ramp, m, wp.output_size, interp, 'constant', 255.0)
            assert np.array_equal(got, want), (t, interp)


def test_nonpositive_z_and_nan_give_fill():
    img = np.random.default_rng(5).random((20, 30, 3)).astype(F32)
    # Z = 8 - u: zero at column 8, negative to its right
    m = homography_map([[1, 0, 0], [0, 1, 0], [-1, 0, 8]])
    sx, sy, outside = coords_ref(m, 16, 10)
    assert outside[:, 8:].all() and not outside[:, :8].any()
    for border in ('constant', 'replicate'):
        out = warp_ref(img, m, (16, 10), 'bicubic', border, 0.25)
        assert (out[:, 8:] == F32(0.25)).all() and np.isfinite(out).all()
    # x*x overflows from column 1 on: r2 = inf, 0 * inf = NaN in tx
    m = homography_map([[1e30, 0, 0], [0, 1, 0], [0, 0, 1]])
    sx, sy, outside = coords_ref(m, 16, 10)
    assert np.isnan(sx[:, 1:]).all() and outside[:, 1:].all() and not outside[:, 0].any()
    out = warp_ref((img * 255).astype(np.uint8), m, (16, 10), 'bilinear', 'replicate', 7.0)
    assert (out[:, 1:] == 7).all()
    # an infinite coordinate (fx * xd overflows) is outside as well
    m = homography_map(np.eye(3))
    m[9] = 3e38
    sx, sy, outside = coords_ref(m, 16, 10)
    assert np.isinf(sx[:, 2:]).all() and outside[:, 2:].all() and not outside[:, :2].any()
