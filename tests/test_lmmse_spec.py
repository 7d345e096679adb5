"""CPU-only: the NumPy restatement of the LMMSE demosaic (tests/lmmse_spec.py, the bits tests/test_gpu_lmmse.py asks of the device)
held to three things:

  * literal per-site Python loops written from include/tdk_hip_lmmse.h alone, which take every plane at a reflected position as its
    value at the folded index (the restatement evaluates the formulas at the reflected position instead: the header says both give
    the same bits, and here that is checked), on frames down to 2 x 2 and narrower than the apron, every pattern, both domains;
  * the header's identities: the own colour passes through, a constant mosaic comes back in the linear domain, flips, and no
    dependence on where the frame's samples lie on the extended grid;
  * its purpose: on a synthetic scene with Poisson-Gaussian noise the error to the true frame and the error of the colour differences
    are below RCD's at every noise level, and so is the chroma noise left on a flat grey patch.

Figures of the purpose test (float32 restatement, 256 x 256 RGGB, interior cropped by 14, seed 7), LMMSE / RCD:
  (a, b) = (0, 0):        RMS 0.02874 / 0.03067 (x 0.937)   chroma 0.03048 / 0.03625 (x 0.841)
  (a, b) = (4e-4, 1e-5):  RMS 0.03161 / 0.03398 (x 0.930)   chroma 0.03155 / 0.03807 (x 0.829)   flat-patch chroma 0.00494 / 0.00724 (x 0.682)
  (a, b) = (2e-3, 1e-4):  RMS 0.04157 / 0.04454 (x 0.933)   chroma 0.03545 / 0.04515 (x 0.785)   flat-patch chroma 0.01192 / 0.01730 (x 0.689)
PPG and bilinear are behind RCD in every one of these cells.  The scene is harsher than a photograph (a chirp down to a period of 3
pixels, a checker), hence the size of the errors; the flat-patch figures do not depend on it.  The assertions are "strictly below",
not these figures."""
import numpy as np
import pytest

import lmmse_spec as spec

F = np.float32
PATTERN_IDS = list(spec.PATTERNS)


# ---------------------------------------------------------------- literal loops
def fold1(i, n):
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def literal(mosaic, pattern, flags):
    """include/tdk_hip_lmmse.h, one site and one operation at a time; float32 output of a float32 mosaic."""
    m = np.asarray(mosaic, F)
    h, w = m.shape
    linear = bool(flags & spec.LINEAR)
    g = [F(float.fromhex(v)) for v in ('0x1.a22092p-3', '0x1.70fefap-3', '0x1.fb36c8p-4', '0x1.0f7df8p-4', '0x1.c4b2eep-6')]   # the header's literals
    ninth, eps = F(float.fromhex('0x1.c71c72p-4')), F(float.fromhex('0x1.ad7f2ap-24'))
    half, quarter, zero = F(0.5), F(0.25), F(0)

    def colour(y, x):
        return int(spec.cfa_color(y, x, pattern))

    def plane(values):
        """a plane on the frame's sites, read at any position through the folded index"""
        return lambda y, x: values[fold1(y, h)][fold1(x, w)]

    with np.errstate(all='ignore'):
        t = plane([[m[y, x] if linear else np.sqrt(max(m[y, x], zero)) for x in range(w)] for y in range(h)])

        def estimate(y, x, dy, dx):
            e = (half * (t(y - dy, x - dx) + t(y + dy, x + dx)) - quarter * (t(y - 2 * dy, x - 2 * dx) + t(y + 2 * dy, x + 2 * dx))) + half * t(y, x)
            return t(y, x) - e if colour(y, x) == 1 else e - t(y, x)

        def lowpass(d, y, x, dy, dx):
            p = g[0] * d(y, x)
            for k in range(1, 5):
                p = p + g[k] * (d(y - k * dy, x - k * dx) + d(y + k * dy, x + k * dx))
            return p

        def window(a):   # a: offset -> value
            s = a(0)
            for k in range(1, 5):
                s = s + (a(-k) + a(k))
            return s

        def direction(d, p, y, x, dy, dx):
            mu = window(lambda k: p(y + k * dy, x + k * dx)) * ninth
            vx = eps + window(lambda k: (p(y + k * dy, x + k * dx) - mu) * (p(y + k * dy, x + k * dx) - mu))
            vn = eps + window(lambda k: (d(y + k * dy, x + k * dx) - p(y + k * dy, x + k * dx)) * (d(y + k * dy, x + k * dx) - p(y + k * dy, x + k * dx)))
            return (p(y, x) * vn + d(y, x) * vx) / (vx + vn), (vx * vn) / (vx + vn)

        sites = [(y, x) for y in range(h) for x in range(w)]
        dh = plane([[estimate(y, x, 0, 1) for x in range(w)] for y in range(h)])
        dv = plane([[estimate(y, x, 1, 0) for x in range(w)] for y in range(h)])
        ph = plane([[lowpass(dh, y, x, 0, 1) for x in range(w)] for y in range(h)])
        pv = plane([[lowpass(dv, y, x, 1, 0) for x in range(w)] for y in range(h)])
        Dv = [[None] * w for _ in range(h)]
        for y, x in sites:
            if colour(y, x) != 1:
                xh, vh = direction(dh, ph, y, x, 0, 1)
                xv, vv = direction(dv, pv, y, x, 1, 0)
                Dv[y][x] = (xh * vv + xv * vh) / (vh + vv)
        D = plane(Dv)

        def finish(c):
            if linear:
                return c
            q = max(c, zero)
            return q * q

        out = np.empty((h, w, 3), F)
        for y, x in sites:
            c = colour(y, x)
            if c == 1:
                G = t(y, x)
                along = finish(G - half * (D(y, x - 1) + D(y, x + 1)))
                across = finish(G - half * (D(y - 1, x) + D(y + 1, x)))
                row = colour(y, x + 1)
                out[y, x, 1], out[y, x, row], out[y, x, 2 - row] = m[y, x], along, across
            else:
                G = t(y, x) + D(y, x)
                other = finish(G - quarter * ((D(y - 1, x - 1) + D(y - 1, x + 1)) + (D(y + 1, x - 1) + D(y + 1, x + 1))))
                out[y, x, c], out[y, x, 1], out[y, x, 2 - c] = m[y, x], finish(G), other
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def same_bits(a, b):
    """every bit, dtype and shape (the sign of a zero cannot differ either: an estimated value of the square-root domain is q*q, +0)"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def frame(h, w, seed, kind='random'):
    rng = np.random.default_rng(seed)
    if kind == 'random':
        return rng.uniform(0.0, 1.0, (h, w)).astype(F)
    if kind == 'signed':   # negative samples, zeros, values above 1
        m = rng.uniform(-0.5, 4.0, (h, w)).astype(F)
        m[rng.uniform(size=(h, w)) < 0.2] = 0.0
        return m
    y, x = np.mgrid[0:h, 0:w]
    return (0.1 + 0.05 * x + 0.02 * y + rng.normal(0.0, 0.01, (h, w))).astype(F)   # a noisy ramp


LITERAL_SHAPES = [(2, 2), (3, 2), (2, 5), (7, 5), (13, 11), (4, 13)]   # (height, width): 2 x 2, odd, narrower than the apron


@pytest.mark.parametrize('pattern', PATTERN_IDS)
@pytest.mark.parametrize('flags', [0, spec.LINEAR], ids=['sqrt', 'linear'])
def test_restatement_equals_literal_loops(pattern, flags):
    for n, (h, w) in enumerate(LITERAL_SHAPES):
        for kind in ('random', 'signed', 'ramp'):
            m = frame(h, w, 100 * n + len(kind), kind)
            want = literal(m, spec.PATTERNS[pattern], flags)
            got = spec.lmmse(m, spec.PATTERNS[pattern], flags)
            assert same_bits(got, want), (pattern, flags, h, w, kind, np.abs(got - want).max())


def test_constants_of_the_header():
    assert [float(v).hex() for v in spec.G] == ['0x1.a220920000000p-3', '0x1.70fefa0000000p-3', '0x1.fb36c80000000p-4', '0x1.0f7df80000000p-4', '0x1.c4b2ee0000000p-6']
    assert float(spec.NINTH).hex() == '0x1.c71c720000000p-4' and float(spec.EPS).hex() == '0x1.ad7f2a0000000p-24'
    assert float(spec.G[0] + 2 * (spec.G[1] + spec.G[2] + spec.G[3] + spec.G[4])) == pytest.approx(1.0, abs=1e-7)
    assert spec.APRON == 11
    assert [int(spec.fold(i, 4)) for i in range(-7, 11)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert [int(spec.fold(i, 2)) for i in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert all(int(spec.fold(i, n)) == fold1(i, n) for n in (2, 3, 7, 12) for i in range(-30, 45))


# ---------------------------------------------------------------- the header's identities
@pytest.mark.parametrize('pattern', PATTERN_IDS)
@pytest.mark.parametrize('flags', [0, spec.LINEAR], ids=['sqrt', 'linear'])
def test_own_colour_passes_through(pattern, flags):
    p = spec.PATTERNS[pattern]
    m = frame(21, 18, 5, 'signed')
    m[3, 4], m[4, 4], m[3, 5], m[4, 5] = -0.0, -0.0, -0.0, -0.0
    for src in (m, m.astype(np.float16)):
        out = spec.lmmse(src, p, flags)
        assert out.dtype == src.dtype
        y, x = np.mgrid[0:21, 0:18]
        own = np.take_along_axis(out, spec.cfa_color(y, x, p)[:, :, None], axis=2)[:, :, 0]
        assert np.array_equal(bits(own), bits(src))
    assert spec.lmmse(m, p, flags, np.float16).dtype == np.float16
    assert spec.lmmse(m.astype(np.float16), p, flags, np.float32).dtype == np.float32


@pytest.mark.parametrize('pattern', PATTERN_IDS)
def test_constant_mosaic_comes_back_in_the_linear_domain(pattern):
    for value in (0.0, 0.2, 1.0, 63.7, 1e-3):
        for h, w in ((2, 2), (9, 12), (40, 37)):
            m = np.full((h, w), value, F)
            out = spec.lmmse(m, spec.PATTERNS[pattern], spec.LINEAR)
            assert np.array_equal(bits(out), bits(np.repeat(m[:, :, None], 3, axis=2))), (value, h, w)


@pytest.mark.parametrize('pattern', PATTERN_IDS)
@pytest.mark.parametrize('flags', [0, spec.LINEAR], ids=['sqrt', 'linear'])
def test_flips(pattern, flags):
    p = spec.PATTERNS[pattern]
    for h, w in ((16, 22), (17, 22), (16, 23), (5, 3)):
        m = frame(h, w, h * w, 'signed')
        out = spec.lmmse(m, p, flags)
        flipped = spec.lmmse(m[:, ::-1].copy(), spec.flip_pattern(p, True, w), flags)
        assert same_bits(np.ascontiguousarray(flipped[:, ::-1]), out), ('horizontal', h, w)
        flipped = spec.lmmse(m[::-1].copy(), spec.flip_pattern(p, False, h), flags)
        assert same_bits(np.ascontiguousarray(flipped[::-1]), out), ('vertical', h, w)


def test_a_site_depends_on_the_apron_and_no_further():
    """Tile independence on the restatement's side: a site of a window cut out with an apron's margin has the bits it has in the
    frame, whatever lies beyond."""
    m = frame(64, 70, 3)
    full = spec.lmmse(m, spec.RGGB, 0)
    a = spec.APRON
    for y0, x0 in ((0, 0), (12, 20), (22, 14)):   # even offsets keep the pattern
        part = spec.lmmse(m[y0:y0 + 40, x0:x0 + 42].copy(), spec.RGGB, 0)
        ys = slice(a if y0 else 0, 40 - a)
        xs = slice(a if x0 else 0, 42 - a)
        assert same_bits(np.ascontiguousarray(part[ys, xs]), np.ascontiguousarray(full[y0:y0 + 40, x0:x0 + 42][ys, xs])), (y0, x0)


# ---------------------------------------------------------------- its purpose
N, CROP, SEED = 256, 14, 7
LEVELS = [(0.0, 0.0), (4e-4, 1e-5), (2e-3, 1e-4)]


def true_scene():
    """256 x 256 RGB: sinusoids, a chirp, slanted bars, a checker and tinted patches, within [0.02, 0.95]."""
    y, x = np.mgrid[0:N, 0:N].astype(np.float64)
    half = N // 2
    lum = np.empty((N, N))
    q = (slice(0, half), slice(0, half))
    lum[q] = 0.45 + 0.2 * np.sin(2 * np.pi * x[q] / 9.0) * np.cos(2 * np.pi * y[q] / 13.0) + 0.1 * np.sin(2 * np.pi * (x[q] + y[q]) / 5.0)
    q = (slice(0, half), slice(half, N))
    r2 = (x[q] - half) ** 2 + y[q] ** 2
    lum[q] = 0.45 + 0.3 * np.cos(np.pi * r2 / 380.0)                                   # a chirp: period 3.0 pixels at its far corner
    q = (slice(half, N), slice(0, half))
    lum[q] = 0.45 + 0.35 * np.tanh(3.0 * np.sin(2 * np.pi * (x[q] + 0.37 * y[q]) / 11.0))   # slanted bars
    q = (slice(half, N), slice(half, N))
    lum[q] = 0.3 + 0.4 * (((x[q] // 8) + (y[q] // 8)) % 2)                              # a checker
    tint = np.stack([1.0 + 0.25 * np.sin(2 * np.pi * (x + 2 * y) / 97.0), np.ones((N, N)), 1.0 + 0.25 * np.cos(2 * np.pi * (2 * x - y) / 83.0)], axis=2)
    rgb = lum[:, :, None] * tint
    for (py, px, colour) in ((200, 150, (0.8, 0.3, 0.2)), (150, 200, (0.2, 0.5, 0.8)), (40, 40, (0.6, 0.6, 0.15)), (210, 40, (0.3, 0.7, 0.4))):
        rgb[py:py + 28, px:px + 28] = colour                                             # tinted patches
    return np.clip(rgb, 0.02, 0.95)


def sample(rgb, pattern):
    y, x = np.mgrid[0:rgb.shape[0], 0:rgb.shape[1]]
    return np.take_along_axis(rgb, spec.cfa_color(y, x, pattern)[:, :, None], axis=2)[:, :, 0]


def noisy(clean, a, b, rng):
    return (clean + rng.normal(size=clean.shape) * np.sqrt(a * clean + b)).astype(F)


def errors(rgb, truth):
    c = (slice(CROP, -CROP), slice(CROP, -CROP))
    e = rgb[c].astype(np.float64) - truth[c]
    chroma = np.stack([e[..., 0] - e[..., 1], e[..., 2] - e[..., 1]], axis=2)
    return float(np.sqrt(np.mean(e ** 2))), float(np.sqrt(np.mean(chroma ** 2)))


@pytest.fixture(scope='module')
def purpose(oracle):
    """{(a, b): {method: (RMS, chroma, flat-patch chroma)}}, computed once."""
    truth, flat = true_scene(), np.full((N, N, 3), 0.2)
    rng = np.random.default_rng(SEED)
    table = {}
    for a, b in LEVELS:
        m, f = noisy(sample(truth, spec.RGGB), a, b, rng), noisy(sample(flat, spec.RGGB), a, b, rng)
        methods = {'lmmse': lambda v: spec.lmmse(v, spec.RGGB, 0), 'linear': lambda v: spec.lmmse(v, spec.RGGB, spec.LINEAR),
                   'rcd': lambda v: oracle.rcd(v, oracle.RGGB), 'ppg': lambda v: oracle.ppg(v, oracle.RGGB), 'bilinear': lambda v: oracle.bilinear5x5(v, oracle.RGGB)}
        table[(a, b)] = {name: (*errors(fn(m), truth), errors(fn(f), flat)[1]) for name, fn in methods.items()}
        for name, row in table[(a, b)].items():
            print(f'(a, b) = ({a:g}, {b:g})  {name:9s} RMS {row[0]:.5f}  chroma {row[1]:.5f}  flat-patch chroma {row[2]:.5f}')
    return table


@pytest.mark.parametrize('level', LEVELS, ids=['clean', 'iso-mid', 'iso-high'])
def test_purpose_better_than_rcd(purpose, level):
    row = purpose[level]
    for other in ('rcd', 'ppg', 'bilinear'):
        assert row['lmmse'][1] < row[other][1], ('chroma', other, row)
    assert row['lmmse'][0] < row['rcd'][0], ('RMS', row)
    assert row['lmmse'][0] < row['ppg'][0], ('RMS', row)
    if level != (0.0, 0.0):
        for other in ('rcd', 'ppg', 'bilinear'):
            assert row['lmmse'][2] < row[other][2], ('flat-patch chroma', other, row)
        assert row['linear'][2] < row['rcd'][2], ('flat-patch chroma, linear domain', row)
