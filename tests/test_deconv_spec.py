"""CPU-only: tests/deconv_spec.py, the NumPy restatement of include/tdk_hip_deconv.h, held to literal per-pixel loops on tiny frames,
to the identities the header states, and to the purpose of the stage."""

import math

import numpy as np
import pytest

import deconv_spec as spec

f32 = np.float32


# ------------------------------------------------------------------ literal loops
def literal(x, taps, iterations, threshold, max_gain, weights):
    """The header read pixel by pixel, every operation on np.float32 scalars."""
    h, w, channels = x.shape
    radius = len(taps) - 1
    tiny = f32(2.0 ** -20)

    def at(p, y, xx):
        return p[min(max(y, 0), h - 1)][min(max(xx, 0), w - 1)]

    def blur(s):
        hor = [[None] * w for _ in range(h)]
        for y in range(h):
            for xx in range(w):
                acc = f32(taps[0]) * s[y][xx]
                for k in range(1, radius + 1):
                    acc = f32(acc + f32(f32(taps[k]) * f32(at(s, y, xx - k) + at(s, y, xx + k))))
                hor[y][xx] = acc
        out = [[None] * w for _ in range(h)]
        for y in range(h):
            for xx in range(w):
                acc = f32(taps[0]) * hor[y][xx]
                for k in range(1, radius + 1):
                    acc = f32(acc + f32(f32(taps[k]) * f32(at(hor, y - k, xx) + at(hor, y + k, xx))))
                out[y][xx] = acc
        return out

    o = [[None] * w for _ in range(h)]
    for y in range(h):
        for xx in range(w):
            px = [f32(v) for v in x[y, xx]]
            if channels == 3:
                lum = f32(f32(f32(f32(weights[0]) * px[0]) + f32(f32(weights[1]) * px[1])) + f32(f32(weights[2]) * px[2]))
            else:
                lum = px[0]
            lum = lum if lum > 0 else f32(0)
            o[y][xx] = max(lum, tiny)
    u = [row[:] for row in o]
    for _ in range(iterations):
        b = blur(u)
        q = [[f32(o[y][xx] / max(b[y][xx], tiny)) for xx in range(w)] for y in range(h)]
        c = blur(q)
        u = [[f32(u[y][xx] * c[y][xx]) for xx in range(w)] for y in range(h)]
    out = np.empty_like(x)
    mask = np.empty((h, w), dtype=f32)
    for y in range(h):
        for xx in range(w):
            if threshold is None:
                m = f32(1)
            else:
                around = [at(o, y + dy, xx + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
                t = f32(threshold)
                it = f32(f32(1) / t)
                d = f32(np.sqrt(max(around)) - np.sqrt(min(around)))
                e = min(max(f32(f32(d - t) * it), f32(0)), f32(1))
                m = f32(f32(e * e) * f32(f32(3) - f32(f32(2) * e)))
            mask[y, xx] = m
            if iterations == 0:
                out[y, xx] = x[y, xx]
                continue
            yn = f32(o[y][xx] + f32(m * f32(u[y][xx] - o[y][xx])))
            g = min(max(f32(yn / o[y][xx]), f32(f32(1) / f32(max_gain))), f32(max_gain))
            for c in range(channels):
                out[y, xx, c] = f32(f32(x[y, xx, c]) * g)   # the assignment rounds to the frame's type
    return out, mask


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_restatement_equals_literal_loops_on_tiny_frames(dtype):
    rng = np.random.default_rng(5)
    cases = [((1, 1), 3, 0.7, 3), ((1, 1), 1, 2.0, 2), ((5, 2), 3, 0.7, 2), ((2, 7), 1, 0.7, 3), ((6, 5), 3, 0.3, 4), ((7, 6), 1, 1.2, 2), ((4, 9), 3, 2.0, 1),
             ((6, 5), 3, 0.7, 0)]
    for (h, w), channels, sigma, iterations in cases:
        taps = spec.gaussian_taps(sigma)
        x = rng.uniform(-0.1, 1.0, (h, w, channels)).astype(dtype)
        x[rng.random((h, w)) < 0.3] *= 0.2   # dark pixels: contrast above and below the threshold
        for threshold in (0.05, None):
            got, m = spec.process(x, taps, iterations, threshold, 2.0, (0.25, 0.625, 0.125))
            want, m_want = literal(x, taps, iterations, threshold, 2.0, (0.25, 0.625, 0.125))
            assert got.dtype == x.dtype and np.array_equal(bits(got), bits(want)), (h, w, channels, sigma, iterations, threshold)
            assert np.array_equal(bits(m), bits(m_want)), (h, w, channels, sigma, iterations, threshold)
    assert any(w < len(spec.gaussian_taps(s)) - 1 for (h, w), _, s, _ in cases)   # a frame narrower than R


def test_taps_follow_the_rule_of_the_sharpener():
    for sigma, radius in ((0.3, 1), (0.5, 2), (0.7, 3), (1.0, 3), (1.2, 4), (1.5, 5), (2.0, 6)):
        taps = spec.gaussian_taps(sigma)
        assert len(taps) == radius + 1 == math.ceil(3.0 * float(f32(sigma))) + 1 and all(t.dtype == f32 for t in taps)
        assert abs(float(taps[0]) + 2.0 * sum(float(t) for t in taps[1:]) - 1.0) < 1e-6
        assert all(taps[k] > taps[k + 1] > 0 for k in range(radius))


# ------------------------------------------------------------------ identities
def test_identities_of_the_header():
    rng = np.random.default_rng(9)
    taps = spec.gaussian_taps(0.7)
    for dtype in (np.float32, np.float16):
        x = rng.uniform(-0.2, 1.0, (11, 13, 3)).astype(dtype)
        x[0, 0] = (-0.0, 0.0, -0.0)
        # N = 0: the input's bits
        out, _ = spec.process(x, taps, 0, 0.02)
        assert np.array_equal(bits(out), bits(x))
        # m = 0 everywhere (a threshold no contrast reaches): g = 1 and the input's bits
        out, m = spec.process(x, taps, 6, 100.0)
        assert not m.any() and np.array_equal(bits(out), bits(x))
        # max_gain 1 holds every pixel
        out, _ = spec.process(x, taps, 6, None, 1.0)
        assert np.array_equal(bits(out), bits(x))
    # the mask is 0 on a flat frame ...
    flat = np.full((9, 9, 3), 0.3, dtype=f32)
    out, m = spec.process(flat, taps, 4, 0.02)
    assert not m.any() and np.array_equal(bits(out), bits(flat))
    # ... and 1 across a step larger than 2t in the square-root domain, 0 two pixels away from it
    t = 1.0 / 64
    step = np.empty((9, 12, 1), dtype=f32)
    step[:, :6], step[:, 6:] = 0.5 ** 2, (0.5 + 2 * t + 1 / 1024) ** 2
    m = spec.contrast_mask(spec.luminance(step), t)
    assert (m[:, 5:7] == 1).all() and not m[:, :4].any() and not m[:, 8:].any()
    step[:, 6:] = (0.5 + t) ** 2   # exactly t: nothing
    assert not spec.contrast_mask(spec.luminance(step), t).any()
    step[:, 6:] = (0.5 + 1.5 * t) ** 2   # halfway: smoothstep(0.5) = 0.5
    assert (spec.contrast_mask(spec.luminance(step), t)[:, 5:7] == 0.5).all()
    # the iteration keeps a flat frame flat to the rounding of the taps' sum
    u = spec.iterate(spec.luminance(flat), taps, 8)
    assert np.abs(u / f32(0.3) - 1).max() < 1e-5


# ------------------------------------------------------------------ purpose
def scene(h=96, w=128):
    yy, xx = np.mgrid[0:h, 0:w]
    s = np.full((h, w), 0.18)
    s[:, w // 2:] = 0.6                                   # a vertical edge
    s[h // 2:, : w // 4] = 0.05                           # a horizontal edge
    s[8:40, 8:56] = 0.3 + 0.15 * ((xx[8:40, 8:56] // 2 + yy[8:40, 8:56] // 2) % 2)   # a fine checkerboard
    s[56:88, 72:120] = 0.45 + 0.12 * np.sin(xx[56:88, 72:120] * 2.1) * np.sin(yy[56:88, 72:120] * 1.7)   # fine texture
    s[60:90, 36:60] = 0.25                                # a flat patch
    return s


def edge_width(profile):
    """The 10-90 % rise of a profile across an edge, by linear interpolation, in pixels."""
    lo, hi = profile[:4].mean(), profile[-4:].mean()
    p = (profile - lo) / (hi - lo)

    def cross(level):
        i = int(np.argmax(p >= level))
        return i - 1 + (level - p[i - 1]) / (p[i] - p[i - 1])

    return cross(0.9) - cross(0.1)


def test_purpose_detail_comes_back_and_flat_noise_stays():
    """A sharp scene (edges, a checkerboard, fine texture, a flat patch) blurred by the Gaussian of sigma 0.7 with Poisson-Gaussian
    noise of variance 2e-5 x + 1e-6 on top; the defaults (sigma 0.7, N = 8, threshold 0.02, max_gain 4).  Measured on this restatement:

        RMS error to the sharp scene      0.0333 -> 0.0229, ratio 0.688 (0.625 without the mask)      asserted < 0.844
        10-90 % width of the edge         2.11 px -> 0.98 px, ratio 0.466                              asserted < 0.733
        noise gain on the flat patch      1.000 with the mask, 1.865 without                            asserted < 1.43 < without
        mean of the flat patch            kept to 1e-5 of its value                                     asserted to 1e-3

    Every bound lies halfway between the measured ratio and 1, "no effect" (for the mask: the unmasked gain).  The threshold: 0.01
    gives the better RMS ratio here (0.617) but lets the patch's noise grow by 6 %, and at four times the noise by 56 %; 0.02 keeps
    the gain at 1.00 and 1.06 while the mask stays 1 on the edge and 0.998 on the checkerboard; 0.04 loses the checkerboard (mask
    0.02).  0.02 stays the default."""
    sigma, iterations, threshold = 0.7, 8, 0.02
    taps = spec.gaussian_taps(sigma)
    sharp = scene()
    h, w = sharp.shape
    rng = np.random.default_rng(4)
    blurred = spec.blur(sharp.astype(f32), taps).astype(np.float64)
    noisy = blurred + rng.normal(0, 1, blurred.shape) * np.sqrt(2e-5 * blurred + 1e-6)
    x = np.repeat(noisy[..., None], 3, axis=2).astype(f32)
    luma = (0.25, 0.5, 0.25)
    out, m = spec.process(x, taps, iterations, threshold, 4.0, luma)
    unmasked, ones = spec.process(x, taps, iterations, None, 4.0, luma)
    assert (ones == 1).all()
    y, yu = out[..., 1].astype(np.float64), unmasked[..., 1].astype(np.float64)

    inner = (slice(8, -8), slice(8, -8))
    rms = lambda z: float(np.sqrt(((z - sharp)[inner] ** 2).mean()))
    across = (slice(44, 54), slice(w // 2 - 8, w // 2 + 8))
    width = lambda z: float(edge_width(z[across].mean(0)))
    patch = (slice(64, 86), slice(40, 56))
    figures = dict(rms_ratio=rms(y) / rms(noisy), rms_ratio_unmasked=rms(yu) / rms(noisy), width_in=width(noisy), width_ratio=width(y) / width(noisy),
                   gain=y[patch].std() / noisy[patch].std(), gain_unmasked=yu[patch].std() / noisy[patch].std(), mean_ratio=y[patch].mean() / noisy[patch].mean(),
                   mask_patch=float(m[patch].mean()), mask_edge=float(m[44:54, w // 2 - 1: w // 2 + 1].mean()), mask_checker=float(m[10:38, 10:54].mean()))
    print({k: round(float(v), 4) for k, v in figures.items()})
    assert figures['rms_ratio'] < 0.844
    assert figures['width_ratio'] < 0.733
    assert figures['gain'] < 1.43 < figures['gain_unmasked']
    assert abs(figures['mean_ratio'] - 1.0) < 1e-3
    assert figures['mask_patch'] < 0.05 and figures['mask_edge'] == 1.0 and figures['mask_checker'] > 0.95
