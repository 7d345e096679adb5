"""CPU-only: tests/toneequal_spec.py, the NumPy restatement of include/tdk_hip_toneeq.h, held to

  * literal per-pixel loops over the header's formulas on small frames (every cell size, radii 0 to 8, frames smaller than a cell,
    not a multiple of it, grids smaller than the window), bit for bit;
  * its curve: zero gains give a table of exact ones, the correction passes through the nine gains, and the table interpolated as
    the device does stays within the recorded distance of the exact curve;
  * its purpose, on a scene of two halves 5 EV apart with 10 % texture: a 3 EV shadow lift behind the mask brings the halves to 3 EV
    apart and keeps the texture contrast of both, where the same table applied per pixel changes it.

Recorded on this restatement:
  TABLE_DEVIATION  the largest relative deviation of the interpolated table from the exact curve over 2^-10 .. 2 for the steep
                   curve (4, 3, 2, 1, 0, -1, -2, -3, -4): 3.2e-4 at 32 steps per octave; asserted with a factor 2.
  EDGE_DEVIATION   the worst deviation of the column-mean gain from its plateau within 80 columns of the edge: -10.1 % on the dark
                   side (+3.2 % at most on either side); asserted with a factor 1.5."""

import numpy as np
import pytest

import toneequal_spec as spec

f32 = np.float32
TABLE_DEVIATION = 3.2e-4
EDGE_DEVIATION = 0.1015


# ---- literal loops
def loop_tree(v):
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def loop_box(p, r):
    h, w = len(p), len(p[0])
    clamp = lambda v, n: min(max(v, 0), n - 1)  # noqa: E731
    hs = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            acc = p[y][clamp(x - r, w)]
            for k in range(-r + 1, r + 1):
                acc = acc + p[y][clamp(x + k, w)]
            hs[y][x] = acc
    out = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            acc = hs[clamp(y - r, h)][x]
            for k in range(-r + 1, r + 1):
                acc = acc + hs[clamp(y + k, h)][x]
            out[y][x] = acc
    return out


def loop_process(x, table, s, r, eps, weights):
    h, w, _ = x.shape
    xf = x.astype(f32)
    w0, w1, w2 = (f32(v) for v in weights)
    zero = f32(0)
    lum = [[None] * w for _ in range(h)]
    for y in range(h):
        for i in range(w):
            t = (w0 * xf[y, i, 0] + w1 * xf[y, i, 1]) + w2 * xf[y, i, 2]
            lum[y][i] = t if t > 0 else zero
    ch, cw = -(-h // s), -(-w // s)
    cells = [[loop_tree([loop_tree([lum[min(cy * s + j, h - 1)][min(cx * s + i, w - 1)] for i in range(s)]) for j in range(s)]) * f32(1.0 / (s * s))
              for cx in range(cw)] for cy in range(ch)]
    inv, eps = f32(1.0 / float((2 * r + 1) * (2 * r + 1))), f32(eps)
    b1, b2 = loop_box(cells, r), loop_box([[v * v for v in row] for row in cells], r)
    ca, cb = [[None] * cw for _ in range(ch)], [[None] * cw for _ in range(ch)]
    for cy in range(ch):
        for cx in range(cw):
            mean, corr = b1[cy][cx] * inv, b2[cy][cx] * inv
            var = corr - mean * mean
            var = var if var > 0 else zero
            a = var / (var + eps)
            ca[cy][cx], cb[cy][cx] = a, mean - a * mean
    big_a = [[v * inv for v in row] for row in loop_box(ca, r)]
    big_b = [[v * inv for v in row] for row in loop_box(cb, r)]

    def axis(p, n):
        q = max(2 * p + 1 - s, 0)
        c0 = q // (2 * s)
        return c0, min(c0 + 1, n - 1), f32(q % (2 * s)) / f32(2 * s)

    def lerp(p0, p1, f):
        return p0 + f * (p1 - p0)

    out, mask = np.zeros((h, w, 3), dtype=x.dtype), np.zeros((h, w), dtype=f32)
    lo, hi = f32(2.0 ** -16), np.nextafter(f32(16), f32(0))
    for y in range(h):
        y0, y1, fy = axis(y, ch)
        for i in range(w):
            x0, x1, fx = axis(i, cw)
            au = lerp(lerp(big_a[y0][x0], big_a[y0][x1], fx), lerp(big_a[y1][x0], big_a[y1][x1], fx), fy)
            bu = lerp(lerp(big_b[y0][x0], big_b[y0][x1], fx), lerp(big_b[y1][x0], big_b[y1][x1], fx), fy)
            m = au * lum[y][i] + bu
            mask[y, i] = m
            mc = min(max(m, lo), hi)
            bits = int(np.array(mc, dtype=f32).view(np.uint32))
            e, mant = (bits >> 23) - 127, bits & 0x7FFFFF
            k = (e + 16) * 32 + (mant >> 18)
            f = f32(mant & 0x3FFFF) / f32(262144)
            g = table[k] + f * (table[k + 1] - table[k])
            for c in range(3):
                out[y, i, c] = xf[y, i, c] * g
    return out, mask


def frame(h, w, seed, dtype=f32):
    rng = np.random.default_rng(seed)
    x = np.exp2(rng.uniform(-12, 3, (h, w, 3))) * np.where(rng.random((h, w, 3)) < 0.05, -1.0, 1.0)
    return x.astype(dtype)


@pytest.mark.parametrize('h,w,cell,radius,eps,dtype', [
    (1, 1, 2, 0, 1e-4, f32), (3, 5, 8, 2, 1e-4, f32), (9, 13, 4, 1, 1e-8, f32), (18, 21, 2, 3, 1e-4, np.float16), (17, 33, 16, 8, 1.0, f32), (12, 8, 4, 8, 1e-4, np.float16),
])
def test_restatement_equals_literal_loops(h, w, cell, radius, eps, dtype):
    x = frame(h, w, h * 100 + w, dtype)
    table = spec.make_table((3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0), mask_exposure=-2.0)
    weights = (0.3, 0.6, 0.1) if cell == 4 else spec.REC709
    out, m = spec.process(x, table, cell, radius, eps, weights)
    want_out, want_m = loop_process(x, table, cell, radius, eps, weights)
    assert out.dtype == x.dtype and m.dtype == f32
    assert np.array_equal(m.view(np.uint32), want_m.view(np.uint32))
    assert np.array_equal(out.view(np.uint8), want_out.view(np.uint8))


def test_lookup_covers_both_clamps_and_every_node():
    table = spec.make_table((1, 0.5, 0, 0, 0, 0, 0, -0.5, -1))
    assert table.shape == (641,) and table.dtype == f32
    nodes = spec.nodes().astype(f32)
    assert np.array_equal(spec.gain(nodes[:-1], table), table[:-1])       # a node returns its entry; the last is never reached
    assert spec.gain(np.array([0, 1e-30, 2.0 ** -17], dtype=f32), table).tolist() == [table[0]] * 3
    top = spec.gain(np.array([16, 1e30], dtype=f32), table)
    assert top[0] == top[1] and table[639] >= top[0] >= table[640]


def test_zero_gains_give_a_table_of_exact_ones():
    assert np.array_equal(spec.make_table((0,) * 9), np.ones(641, dtype=f32))
    assert np.array_equal(spec.make_table((0,) * 9, mask_exposure=3.5), np.ones(641, dtype=f32))
    x = frame(9, 13, 7)
    out, _ = spec.process(x, spec.make_table((0,) * 9), 4, 2)
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32))


def test_curve_passes_through_the_nine_gains():
    for gains in ((3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0), (4, 3, 2, 1, 0, -1, -2, -3, -4), (0, 0, 0, 0, 2, 0, 0, 0, 0)):
        w = spec.curve(gains)
        assert np.abs(spec.correction(spec.CENTRES, w) - np.asarray(gains)).max() < 1e-12
        # outside the bands the correction is that of the nearest band
        assert spec.correction(np.array([-12.0, 3.0]), w).tolist() == spec.correction(np.array([-8.0, 0.0]), w).tolist()
    # mask_exposure shifts the mask in front of the curve
    shifted = spec.make_table((3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0), mask_exposure=1.0)
    assert np.array_equal(shifted[:-32], spec.make_table((3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0))[32:])


def test_interpolated_table_stays_near_the_exact_curve():
    gains = (4, 3, 2, 1, 0, -1, -2, -3, -4)
    table, w = spec.make_table(gains), spec.curve(gains)
    m = np.exp(np.random.default_rng(0).uniform(np.log(2.0 ** -10), np.log(2.0), 200000)).astype(f32)
    exact = 2.0 ** spec.correction(np.log2(m.astype(np.float64)), w)
    deviation = np.abs(spec.gain(m, table).astype(np.float64) / exact - 1).max()
    print(f'table deviation {deviation:.3e} (recorded {TABLE_DEVIATION:.1e})')
    assert deviation <= 2 * TABLE_DEVIATION


# ---- the purpose
H, W = 384, 512
GAINS = (3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0)


@pytest.fixture(scope='module')
def scene():
    rng = np.random.default_rng(1)
    texture = 1 + 0.2 * np.sin(np.arange(W)[None, :] * 0.9) * np.sin(np.arange(H)[:, None] * 0.7) + 0.03 * rng.standard_normal((H, W))
    base = np.where(np.arange(W)[None, :] < W // 2, 2.0 ** -7, 2.0 ** -2) * np.ones((H, 1))
    lum = (base * texture).astype(f32)
    table = spec.make_table(GAINS)
    weights = (0.25, 0.5, 0.25)   # exact on a grey frame: the luminance is the value
    out, _ = spec.process(np.repeat(lum[..., None], 3, axis=2), table, 8, 4, 1e-4, weights)
    assert np.array_equal(spec.luminance(np.repeat(lum[..., None], 3, axis=2), weights), lum)
    return lum.astype(np.float64), out[..., 0].astype(np.float64), lum.astype(np.float64) * spec.gain(lum, table)


def halves(img):
    """(EV between the means of the halves, contrast of the dark half, of the bright half): 40 columns clear of the borders, 80 of the edge."""
    dark, bright = img[:, 40:W // 2 - 80], img[:, W // 2 + 80:W - 40]
    return np.log2(bright.mean() / dark.mean()), dark.std() / dark.mean(), bright.std() / bright.mean()


def test_shadow_lift_keeps_the_texture_of_both_halves(scene):
    lum, guided, per_pixel = scene
    ev_in, dark_in, bright_in = halves(lum)
    ev, dark, bright = halves(guided)
    print(f'in {ev_in:.3f} EV, contrast {dark_in:.4f} {bright_in:.4f}; guided {ev:.3f} EV, contrast {dark:.4f} {bright:.4f}')
    assert abs(ev_in - 5.0) < 0.01
    assert abs(ev - 3.0) <= 0.05
    assert abs(dark / dark_in - 1) <= 0.05 and abs(bright / bright_in - 1) <= 0.05
    ev_pp, dark_pp, bright_pp = halves(per_pixel)
    print(f'per pixel {ev_pp:.3f} EV, contrast {dark_pp:.4f} {bright_pp:.4f}')
    assert abs(ev_pp - 3.0) <= 0.05   # the same tones ...
    assert max(abs(dark_pp / dark_in - 1), abs(bright_pp / bright_in - 1)) > 0.09   # ... but not the same texture


def test_gain_next_to_the_edge_stays_near_its_plateau(scene):
    lum, guided, _ = scene
    gain = (guided / lum).mean(0)
    plateau_dark, plateau_bright = gain[40:W // 2 - 80].mean(), gain[W // 2 + 80:W - 40].mean()
    assert abs(plateau_dark / 8.0 - 1) < 0.01 and abs(plateau_bright / 2.0 - 1) < 0.01
    dark, bright = gain[W // 2 - 80:W // 2] / plateau_dark - 1, gain[W // 2:W // 2 + 80] / plateau_bright - 1
    worst = max(np.abs(dark).max(), np.abs(bright).max())
    print(f'dark side {dark.min():+.4f} .. {dark.max():+.4f}, bright side {bright.min():+.4f} .. {bright.max():+.4f} (recorded {EDGE_DEVIATION})')
    assert worst <= 1.5 * EDGE_DEVIATION
