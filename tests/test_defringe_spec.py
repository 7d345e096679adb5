"""CPU-only: tests/defringe_spec.py, the NumPy restatement of include/tdk_hip_defringe.h, held to literal per-pixel loops on tiny
frames, to the identities the header states, and to the purpose of the stage."""

import math

import numpy as np
import pytest

import defringe_spec as spec

f32 = np.float32


def bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ------------------------------------------------------------------ literal loops
def literal(x, taps, sample_radius, strength, floor, mode, domain):
    """The header read pixel by pixel, every operation on np.float32 scalars."""
    h, w, _ = x.shape
    radius = len(taps) - 1

    def at(p, y, xx):
        return p[min(max(y, 0), h - 1)][min(max(xx, 0), w - 1)]

    def blur(s):
        hor = [[None] * w for _ in range(h)]
        for y in range(h):
            for xx in range(w):
                acc = f32(f32(taps[0]) * s[y][xx])
                for k in range(1, radius + 1):
                    acc = f32(acc + f32(f32(taps[k]) * f32(at(s, y, xx - k) + at(s, y, xx + k))))
                hor[y][xx] = acc
        out = [[None] * w for _ in range(h)]
        for y in range(h):
            for xx in range(w):
                acc = f32(f32(taps[0]) * hor[y][xx])
                for k in range(1, radius + 1):
                    acc = f32(acc + f32(f32(taps[k]) * f32(at(hor, y - k, xx) + at(hor, y + k, xx))))
                out[y][xx] = acc
        return out

    lum, cb, cr = ([[None] * w for _ in range(h)] for _ in range(3))
    for y in range(h):
        for xx in range(w):
            t = []
            for c in range(3):
                v = f32(x[y, xx, c])
                v = v if v > 0 else f32(0)
                t.append(f32(np.sqrt(v)) if domain == 'sqrt' else v)
            lum[y][xx] = f32(f32(f32(f32(0.25) * t[0]) + f32(f32(0.5) * t[1])) + f32(f32(0.25) * t[2]))
            cb[y][xx] = f32(t[2] - t[1])
            cr[y][xx] = f32(t[0] - t[1])
    gb, gr = blur(cb), blur(cr)
    e = [[None] * w for _ in range(h)]
    total = 0
    for y in range(h):
        for xx in range(w):
            db, dr = f32(cb[y][xx] - gb[y][xx]), f32(cr[y][xx] - gr[y][xx])
            e[y][xx] = f32(f32(db * db) + f32(dr * dr))
            total += int(math.floor(float(f32(min(e[y][xx], f32(1024.0)) * f32(1048576.0)))))
    assert total < 2 ** 64
    if mode == 'static':
        th = max(f32(floor), f32(strength))
    else:
        avg = f32(np.float64(total) / (np.float64(w * h) * np.float64(1048576.0)))
        th = max(f32(floor), f32(f32(strength) * avg))
    out = x.copy()
    mask = np.zeros((h, w), dtype=np.uint8)
    for y in range(h):
        for xx in range(w):
            if not e[y][xx] > th:
                continue
            mask[y, xx] = 1
            a = b = n = f32(0)
            for dy in range(-sample_radius, sample_radius + 1):
                for dx in range(-sample_radius, sample_radius + 1):
                    if dx * dx + dy * dy > sample_radius * sample_radius:
                        continue
                    wt = f32(f32(1.0) / f32(at(e, y + dy, xx + dx) + th))
                    a = f32(a + f32(wt * at(cb, y + dy, xx + dx)))
                    b = f32(b + f32(wt * at(cr, y + dy, xx + dx)))
                    n = f32(n + wt)
            cb2, cr2 = f32(a / n), f32(b / n)
            g = f32(lum[y][xx] - f32(f32(0.25) * f32(cb2 + cr2)))
            for c, v in enumerate((f32(g + cr2), g, f32(g + cb2))):
                v = max(v, f32(0))
                out[y, xx, c] = f32(v * v) if domain == 'sqrt' else v   # the assignment rounds to the frame's type
    return out, mask, np.array(e, dtype=f32).reshape(h, w), total, th


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_restatement_equals_literal_loops_on_tiny_frames(dtype):
    rng = np.random.default_rng(5)
    # ((h, w), taps, S_r, strength, mode, domain); R and S_r larger than the frame are among them
    cases = [((1, 1), spec.gaussian_taps(2.0), 6, 2.5, 'global', 'sqrt'), ((3, 5), spec.gaussian_taps(4.0), 8, 1.0, 'global', 'sqrt'),
             ((9, 12), spec.gaussian_taps(0.5), 1, 0.5, 'global', 'linear'), ((7, 6), (f32(0.5), f32(0.25)), 3, 1.5, 'global', 'sqrt'),
             ((9, 12), spec.gaussian_taps(1.0), 4, 0.01, 'static', 'sqrt'), ((2, 7), spec.gaussian_taps(2.0), 8, 0.002, 'static', 'linear'),
             ((6, 5), spec.gaussian_taps(1.0), 2, 0.0, 'global', 'sqrt')]
    changed = 0
    for (h, w), taps, s_r, strength, mode, domain in cases:
        x = rng.uniform(-0.1, 1.0, (h, w, 3)).astype(dtype)
        x[rng.random((h, w)) < 0.3] *= 0.1
        if h * w > 1:
            x[0, 0] = (-0.0, 0.0, -0.5)
        got = spec.process(x, taps, s_r, strength, 1e-4, mode, domain)
        want = literal(x, taps, s_r, strength, 1e-4, mode, domain)
        key = (h, w, len(taps) - 1, s_r, strength, mode, domain)
        assert got[0].dtype == x.dtype and np.array_equal(bits(got[0]), bits(want[0])), key
        assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2])), key
        assert got[3] == want[3] and bits(np.asarray(got[4], dtype=f32)) == bits(np.asarray(want[4], dtype=f32)), key
        changed += int(got[1].sum())
        assert h * w == 1 or 0 < got[1].sum() < h * w or strength == 0.0, key   # both kinds of pixel
    assert changed > 40
    assert any(w < len(t) - 1 and w < s for (h, w), t, s, *_ in cases)   # a frame narrower than R and than S_r


def test_taps_follow_the_rule_of_the_sharpener():
    for sigma, radius in ((0.5, 2), (0.7, 3), (1.0, 3), (1.5, 5), (2.0, 6), (3.0, 9), (3.7, 12), (4.0, 12)):
        taps = spec.gaussian_taps(sigma)
        assert len(taps) == radius + 1 == math.ceil(3.0 * float(f32(sigma))) + 1 and all(t.dtype == f32 for t in taps)
        assert abs(float(taps[0]) + 2.0 * sum(float(t) for t in taps[1:]) - 1.0) < 1e-6
        assert all(taps[k] > taps[k + 1] > 0 for k in range(radius))


def test_disc_is_visited_row_by_row():
    assert spec.disc(1) == [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]
    for r in range(1, 9):
        d = spec.disc(r)
        assert d == sorted(d) and len(set(d)) == len(d) and (0, 0) in d and (0, r) in d and (-r, 0) in d
        assert all(dx * dx + dy * dy <= r * r for dy, dx in d) and len(d) == sum(1 for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r)
    assert [len(spec.disc(r)) for r in (1, 6, 8)] == [5, 113, 197]


# ------------------------------------------------------------------ identities
def test_identities_of_the_header():
    rng = np.random.default_rng(9)
    taps = spec.gaussian_taps(2.0)
    for dtype in (np.float32, np.float16):
        for domain in ('sqrt', 'linear'):
            # a flat frame returns its bits: E is 0 for grey and the square of a rounding error otherwise, never greater than a floor of 1e-4
            for value in ((0.3, 0.3, 0.3), (0.9, 0.1, 0.4), (-0.0, -0.25, 64.0)):
                flat = np.empty((9, 11, 3), dtype=dtype)
                flat[:] = value
                for mode, strength in (('global', 2.5), ('global', 0.0), ('static', 0.0)):
                    out, mask, e, s, th = spec.process(flat, taps, 6, strength, 1e-4, mode, domain)
                    assert e.max() < 1e-9 and (value[0] != value[1] or not e.any()) and s == 0 and th == f32(1e-4) and not mask.any() and np.array_equal(bits(out), bits(flat))
            # a static threshold above every E returns the input's bits
            x = rng.uniform(-0.2, 1.0, (11, 13, 3)).astype(dtype)
            x[0, 0] = (-0.0, 0.0, -0.0)
            e = spec.process(x, taps, 6, 0.0, 1e-4, 'static', domain)[2]
            out, mask, _, _, th = spec.process(x, taps, 6, float(e.max()), 1e-4, 'static', domain)
            assert th == e.max() and not mask.any() and np.array_equal(bits(out), bits(x))
            # ... and one just below the largest rewrites exactly that pixel
            out, mask, _, _, _ = spec.process(x, taps, 6, float(np.nextafter(e.max(), f32(0))), 1e-4, 'static', domain)
            assert mask.sum() == 1 and mask.flat[int(e.argmax())] == 1 and (bits(out) != bits(x)).any(axis=2).sum() <= 1


def test_statistic_is_capped_and_order_free():
    e = np.array([[0.0, 1e-7, 0.5], [1024.0, 5000.0, np.inf]], dtype=f32)
    assert spec.statistic(e) == 0 + 0 + (1 << 19) + 3 * (1 << 30)
    assert spec.statistic(np.full((3, 3), 2.0 ** -20, dtype=f32)) == 9 and spec.statistic(np.full((3, 3), np.nextafter(f32(2.0 ** -20), f32(0)), dtype=f32)) == 0
    assert spec.threshold(3 << 30, 3, 2.0, 1e-4) == f32(2048.0) and spec.threshold(0, 5, 2.0, 1e-4) == f32(1e-4)
    assert spec.threshold(123, 7, 0.25, 1e-4, static=True) == f32(0.25) and spec.threshold(123, 7, 0.0, 1e-4, static=True) == f32(1e-4)
    # the largest frame of capped pixels still fits 64 bits
    assert 65535 * 65535 * (1 << 30) < 1 << 64


def test_mirror_identity_holds_for_the_analysis_and_not_for_the_correction():
    """The header claims no mirror identity for the frame.  E, the mask, S and th of a mirrored frame are the mirrored ones; a rewritten
    sample may differ, because the samples of its disc are visited in the opposite order."""
    rng = np.random.default_rng(2)
    taps = spec.gaussian_taps(1.5)
    x = rng.uniform(0.0, 1.0, (24, 28, 3)).astype(f32)
    out, mask, e, s, th = spec.process(x, taps, 4, 1.0)
    differs = 0
    for flip in (lambda a: a[:, ::-1], lambda a: a[::-1]):
        out2, mask2, e2, s2, th2 = spec.process(np.ascontiguousarray(flip(x)), taps, 4, 1.0)
        assert np.array_equal(bits(e2), bits(np.ascontiguousarray(flip(e)))) and np.array_equal(mask2, flip(mask)) and s2 == s and th2 == th
        assert np.allclose(out2, flip(out), rtol=1e-4, atol=1e-6)
        differs += int((bits(out2) != bits(np.ascontiguousarray(flip(out)))).sum())
    assert mask.any() and differs > 0   # the reason the claim was dropped


# ------------------------------------------------------------------ purpose
H = W = 256
SKY_ROWS = 160
PATCHES = [((166, 140), (0.70, 0.08, 0.06)), ((166, 196), (0.08, 0.55, 0.10)), ((210, 140), (0.06, 0.10, 0.70)), ((210, 196), (0.75, 0.65, 0.05))]
PATCH, MARGIN = 40, 14
TEXTURE = (slice(176, 244), slice(12, 116))


def gauss64(plane, sigma):
    """A float64 Gaussian blur of radius ceil(4 sigma), the edge replicated."""
    r = math.ceil(4 * sigma)
    k = np.exp(-np.arange(-r, r + 1) ** 2 / (2.0 * sigma * sigma))
    k /= k.sum()
    for axis in (0, 1):
        padded = np.pad(plane, [(r, r) if a == axis else (0, 0) for a in (0, 1)], mode='edge')
        plane = sum(k[i] * np.take(padded, np.arange(plane.shape[axis]) + i, axis=axis) for i in range(2 * r + 1))
    return plane


def backlit_scene():
    """(the sharp scene in float64, the mask of its dark structures).  A sky at 1.8 times the clip level with dark slanted bars of
    several widths, thin twigs and a ring on it; below it a mid-tone ground with a coloured texture and four saturated patches."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dark = np.zeros((H, W), dtype=bool)
    for x0, slope, width in ((20, 0.15, 2), (50, -0.3, 4), (90, 0.5, 8), (135, -0.1, 3), (170, 0.8, 5), (215, -0.6, 12)):
        dark |= np.abs((xx - x0 - slope * yy) / math.hypot(1.0, slope)) < width / 2
    for y0, slope, width in ((30, 0.2, 1.5), (75, -0.12, 2.5), (120, 0.05, 6)):
        dark |= np.abs((yy - y0 - slope * xx) / math.hypot(1.0, slope)) < width / 2
    dark |= np.abs(np.hypot(xx - 128, yy - 90) - 30) < 1.5
    dark &= yy < SKY_ROWS - 8
    scene = np.empty((H, W, 3))
    scene[:] = (1.8, 1.8, 1.8)
    scene[dark] = (0.05, 0.06, 0.04)
    scene[SKY_ROWS:] = (0.30, 0.32, 0.28)
    ty, tx = TEXTURE
    wave = np.sin(xx[ty, tx] * 0.9) * np.sin(yy[ty, tx] * 0.7)
    scene[ty, tx] = np.stack([0.35 + 0.10 * wave, 0.33 + 0.08 * wave, 0.25 + 0.05 * wave], axis=-1)
    for (py, px), colour in PATCHES:
        scene[py:py + PATCH, px:px + PATCH] = colour
    return scene, dark


def capture(scene, sigmas, rng=None):
    """The scene through a lens that blurs channel c with sigmas[c], Poisson-Gaussian noise of variance 4e-4 x + 1e-5, a sensor that
    clips at 1."""
    x = np.stack([gauss64(scene[..., c], sigmas[c]) for c in range(3)], axis=-1)
    if rng is not None:
        x = x + rng.normal(0, 1, x.shape) * np.sqrt(4e-4 * x + 1e-5)
    return np.clip(x, 0.0, 1.0).astype(f32)


def chroma_rms(x, reference, where):
    _, cb, cr = spec.working(x)
    _, cb0, cr0 = spec.working(reference)
    d = (cb.astype(np.float64) - cb0)[where] ** 2 + (cr.astype(np.float64) - cr0)[where] ** 2
    return float(np.sqrt(d.mean() / 2))


def purpose_figures(defaults=None):
    scene, dark = backlit_scene()
    near = dark
    for _ in range(6):   # within 6 pixels of a dark structure: a 3x3 dilation six times
        near = np.maximum.reduce([spec.shift(spec.shift(near, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    band = near & (np.mgrid[0:H, 0:W][0] < SKY_ROWS - 2)
    reference = capture(scene, (0.8, 0.8, 0.8))
    interior = np.zeros((H, W), dtype=bool)
    for (py, px), _ in PATCHES:
        interior[py + MARGIN:py + PATCH - MARGIN, px + MARGIN:px + PATCH - MARGIN] = True
    texture = np.zeros((H, W), dtype=bool)
    texture[TEXTURE] = True
    kwargs = dict(sigma=2.0, sample_radius=6, strength=2.5, floor=1e-4)
    kwargs.update(defaults or {})
    taps = spec.gaussian_taps(kwargs.pop('sigma'))
    figures = {}
    for name, rng in (('clean', None), ('noisy', np.random.default_rng(11))):
        x = capture(scene, (1.6, 0.8, 2.4), rng)
        out, mask, e, s, th = spec.process(x, taps, **kwargs)
        figures[name] = dict(band_in=chroma_rms(x, reference, band), band_out=chroma_rms(out, reference, band), texture_in=chroma_rms(x, reference, texture),
                             texture_out=chroma_rms(out, reference, texture), rewritten=float(mask.mean()), patches_changed=int((bits(out) != bits(x)).any(axis=2)[interior].sum()),
                             band_share=float(band.mean()), threshold=float(th))
    return figures


def test_purpose_the_halo_shrinks_and_colour_stays():
    """A backlit scene of 256 x 256: a sky at 1.8 times the clip level with dark slanted bars 2 to 12 pixels wide, twigs and a ring;
    below it a mid-tone ground with a coloured texture and four saturated flat patches.  Red is blurred with sigma 1.6, green with
    0.8, blue with 2.4, and the sensor clips at 1; once noise-free and once with Poisson-Gaussian noise of variance 4e-4 x + 1e-5.
    The error is the RMS distance of (Cb, Cr) in the square-root domain to the same scene with every channel at sigma 0.8, over the
    band within 6 pixels of the dark structures (38 % of the frame).  Measured on this restatement with the defaults (sigma 2,
    radius 6, strength 2.5, floor 1e-4, global, sqrt):

                      band error                   texture error            rewritten   patch interiors changed   th
        noise-free    0.1541 -> 0.0900, x 0.584    0.01799 -> 0.01799       9.3 %       0                         0.0140
        noisy         0.1544 -> 0.0906, x 0.587    0.02342 -> 0.02342       9.4 %       0                         0.0145

    (a) the band error falls, asserted strictly and below the measured ratio plus a tenth (0.684, 0.687); (b) the interiors of the
    patches, 14 pixels inside their edges, come back bit for bit; (c) no pixel of the texture is rewritten, so "not above the input"
    holds and is asserted; (d) the share of rewritten pixels is printed and held to the 5 .. 15 % the sweep below stayed in.

    The defaults stayed.  Over sigma 1.5, 2, 3 x radius 4, 6, 8 x strength 1.5, 2.5, 4 the band ratio ran from 0.45 (3, 8, 1.5) to 0.70
    (1.5, 4, 4) and the rewritten share from 5.8 to 14.2 %, no patch interior changed anywhere; strength 1.5 began to rewrite noisy
    texture pixels at sigma 1.5 and 2 (texture ratio 0.994 .. 0.998, harmless here, but it is the noise that sets them off), strength
    2.5 and 4 rewrote none.  A larger sigma or radius lowers the ratio further on this scene (0.51 at sigma 3, 0.56 at radius 8) at
    the price of a wider apron; that is a choice for a lens, not a default."""
    figures = purpose_figures()
    for name, f in figures.items():
        print(name, {k: round(v, 5) for k, v in f.items()}, 'band ratio', round(f['band_out'] / f['band_in'], 4), 'texture ratio', round(f['texture_out'] / f['texture_in'], 4))
    for name, bound in (('clean', 0.684), ('noisy', 0.687)):
        f = figures[name]
        assert f['band_out'] < f['band_in'] and f['band_out'] / f['band_in'] < bound    # (a)
        assert f['patches_changed'] == 0                                              # (b)
        assert f['texture_out'] <= f['texture_in']                                    # (c)
        assert 0.05 < f['rewritten'] < 0.15                                           # (d)
    assert figures['noisy']['texture_out'] - figures['noisy']['texture_in'] <= figures['clean']['texture_in']   # (c) as the issue words it
    assert 0.3 < figures['clean']['band_share'] < 0.5
