"""Input classes and parameter sets of the local Laplacian's whole-domain tests (tests/test_laplacian_spec.py on the CPU,
tests/test_gpu_laplacian_domain.py on the GPU).  Plain numpy; every frame comes from a seeded generator and depends on
(class, height, width) only, so both files -- and both storage types -- see the same data.

A class is (name, maker(h, w) -> float32 (h, w), parameter sets (sigma, shadows, highlights, clarity)).  DESIGN.md "Local Laplacian
over its whole domain" says why each one is there."""

import zlib

import numpy as np

NG = 6
CENTRES = [np.float32((np.float32(k) + np.float32(0.5)) / np.float32(NG)) for k in range(NG)]  # as the kernel and the oracle form them
# the smallest frames that take each branch of the launch schedule (test_gpu_parity.py::test_laplacian_level_schedules)
FRAMES = [(7, 9), (16, 16), (33, 70), (120, 161), (256, 200), (301, 515)]

PLAIN = (0.2, 1.6, 0.7, 0.0)      # clarity 0: the kernel must give the oracle's bits
CLARITY = (0.2, 1.6, 0.7, 0.3)
IDENTITY = (0.2, 1.0, 1.0, 0.0)   # the curve is the identity: a flat frame comes back as its binary16 rounding


def _rng(name, h, w):
    return np.random.default_rng([zlib.crc32(name.encode()), h, w])


def _f16_neighbours(v):
    """binary16 values around fp32 v: the largest below, v itself where it is a binary16 value, the smallest above."""
    h = np.float16(v)
    if np.float32(h) == v:
        return [np.nextafter(h, np.float16(-np.inf)), h, np.nextafter(h, np.float16(np.inf))]
    if np.float32(h) < v:
        return [h, np.nextafter(h, np.float16(np.inf))]
    return [np.nextafter(h, np.float16(-np.inf)), h]


def uniform(lo, hi):
    def make(h, w, name=f'uniform[{lo},{hi}]'):
        return _rng(name, h, w).uniform(lo, hi, (h, w)).astype(np.float32)
    return make


def gamma_centres(h, w):
    """The binary16 values on either side of (and on) each centre -- they sit on the search `centre <= v` and on the clamp of the
    blend weight at 0 and 1 -- and values at or beyond the outer centres."""
    vals = [x for g in CENTRES for x in _f16_neighbours(g)] + [np.float16(x) for x in (-0.3, 0.0, 0.05, 0.95, 1.0, 1.3)]
    vals = np.array(vals, np.float16).astype(np.float32)
    assert (vals[-6:-3] <= CENTRES[0]).all() and (vals[-3:] >= CENTRES[-1]).all()
    return _rng('gamma', h, w).choice(vals, (h, w))


def _two_sigma_point(k, side):
    """A binary16 x beyond centre k (side = +1: above, -1: below), sigma = fp32(|x - g_k|) / 2 so that |c| == 2 sigma holds exactly
    at x, and a slope for that side at which the curve's two branches -- equal there in exact arithmetic -- round to DIFFERENT
    binary16 values in fp32: the select `fabsf(c) > 2 sigma` is then visible in the stored level-0 gamma value.  x lies between
    centre k and its neighbour, so gamma k is one of the two pyramids the assemble blends at that pixel."""
    g = CENTRES[k]
    one, two = np.float32(1.0), np.float32(2.0)
    x = np.float16(g + np.float32(side * 0.04))
    for _ in range(200):
        c = np.float32(x) - g
        sigma = np.abs(c) / two
        ssig = np.copysign(sigma, c)
        for slope in (1.6, 0.7, 0.3, 1.3, 0.45):
            sh = np.float32(slope)
            lin = g + ssig + sh * (c - ssig)
            t = np.minimum(np.maximum(c / (two * ssig), np.float32(0.0)), one)
            bez = g + ssig * two * (one - t) * t + t * t * (ssig + ssig * sh)
            if t == one and np.float16(lin) != np.float16(bez):
                return x, float(sigma), slope
        x = np.nextafter(x, np.float16(side * np.inf))
    raise AssertionError('no discriminating |c| == 2 sigma point')


def two_sigma(k, side):
    x, sigma, slope = _two_sigma_point(k, side)
    prm = (sigma, slope, 0.7, 0.0) if side > 0 else (sigma, 0.7, slope, 0.0)  # c > 0 takes `shadows`, c <= 0 `highlights`

    def make(h, w):
        rng = _rng(f'two_sigma{k}{side}', h, w)
        trio = np.array([np.nextafter(x, np.float16(-np.inf)), x, np.nextafter(x, np.float16(np.inf))], np.float16).astype(np.float32)
        return np.where(rng.random((h, w)) < 0.5, rng.choice(trio, (h, w)), rng.uniform(0, 1, (h, w)).astype(np.float32))
    return make, [prm]


def flat(value):
    def make(h, w):
        return np.full((h, w), value, np.float32)
    return make


FLAT_FIELD, NEAR_CENTRE, LANE_STRIDE = 2.0, 0.42, 97


def wave_sparse(h, w):
    """A field more than 2 sigma from every centre (2.0 at sigma 0.2 and 0.01) with single samples 0.003 from the centre 5/12, 97
    apart in raster order: at most one per 64-lane wave, and waves without one.  Waves without one take the curve's wave-uniform
    shortcut for every gamma, the others leave it for the lanes' sake; at sigma 2.0 no wave takes it."""
    f = np.full(h * w, FLAT_FIELD, np.float32)
    f[5::LANE_STRIDE] = NEAR_CENTRE
    return f.reshape(h, w)


def steps(h, w):
    f = np.zeros((h, w), np.float32)
    f[:, w // 2:] = 1.0
    f[h // 2:, :w // 4] = 1.0
    return f


def scaled(factor):
    def make(h, w):
        return (_rng('scaled', h, w).uniform(0, 1, (h, w)) * factor).astype(np.float32)
    return make


_ts_hi, _ts_hi_prm = two_sigma(2, +1)
_ts_lo, _ts_lo_prm = two_sigma(3, -1)

# (name, maker, parameter sets)
CLASSES = [
    ('uniform_mid', uniform(-0.5, 1.5), [PLAIN, CLARITY]),
    ('uniform_wide', uniform(-8.0, 8.0), [PLAIN, CLARITY, (2.0, 1.4, 0.8, 0.0)]),
    ('gamma_centres', gamma_centres, [PLAIN, (0.1, 0.5, 1.5, 0.3)]),
    ('two_sigma_above', _ts_hi, _ts_hi_prm),
    ('two_sigma_below', _ts_lo, _ts_lo_prm),
    ('flat_0', flat(0.0), [IDENTITY, CLARITY]),
    ('flat_1', flat(1.0), [IDENTITY, CLARITY]),
    ('flat_0.37', flat(0.37), [IDENTITY, CLARITY]),
    ('flat_-3', flat(-3.0), [IDENTITY, CLARITY]),
    ('flat_1000', flat(1000.0), [IDENTITY, CLARITY]),
    ('wave_sparse', wave_sparse, [PLAIN, CLARITY, (0.01, 1.6, 0.7, 0.3), (2.0, 1.6, 0.7, 0.3)]),
    ('steps', steps, [(0.01, 1.6, 0.7, 0.0), (0.01, 1.6, 0.7, 0.3), (2.0, 1.6, 0.7, 0.0), (2.0, 1.6, 0.7, 0.3)]),
    ('tiny', scaled(1e-6), [PLAIN, CLARITY]),             # the binary16 subnormal range
    ('huge', scaled(3e4), [(0.2, 1.0, 0.5, 0.0), (0.2, 0.5, 1.0, 0.0)]),  # slopes <= 1 and no clarity: every curve stays below 65504
]
VALUE_CASES = [(name, make, prm) for name, make, prms in CLASSES for prm in prms]

# the parameter domain, on uniform_mid: every sigma (both sides of the kernel's plain_div range 2^-20 .. 2^20) against clarity 0 and 1,
# every (shadows, highlights) pair and every clarity at least once.  sigma <= 0 is outside the domain (the reference divides by zero).
SIGMAS = [0.01, 0.02, 0.2, 2.0, 2.0 ** -21, 2.0 ** -20, 2.0 ** 20, 2.0 ** 21]
PARAMETER_CASES = ([(s, 1.6, 0.7, c) for s in SIGMAS for c in (0.0, 1.0)]
                   + [(0.2, sh, hl, c) for (sh, hl), c in zip([(0.0, 0.0), (-0.5, 2.5), (2.5, -0.5), (1.0, 1.0)], (0.0, 1.0, -1.0, 5.0))]
                   + [(0.02, 2.5, -0.5, 5.0), (2.0, -0.5, 2.5, -1.0)])

# one non-finite sample in an ordinary frame
SPECIALS = {'nan': np.nan, '+inf': np.inf, '-inf': -np.inf, '7e4': 7e4}   # 7e4 overflows binary16 at the first store
NONFINITE_FRAMES = [(7, 9), (33, 70), (120, 161), (256, 200)]
# ... and with negative and zero slopes at clarity 0: `lin` of an infinite sample is then an infinity of the other sign than the input
# pyramid's (or 0 * inf), which only the reference's always-added clarity term turns into the NaN the result must show
NONFINITE_SLOPES = [(0.2, -0.5, 2.5, 0.0), (0.2, 2.5, -0.5, 0.0), (0.2, 0.0, 0.0, 0.0)]
NONFINITE_SLOPE_FRAMES = [(33, 70), (120, 161)]


def positions(h, w):
    return {'corner00': (0, 0), 'top_mid': (0, w // 2), 'corner11': (h - 1, w - 1), 'interior': (h // 2, w // 2)}


def nonfinite_frame(h, w, special, where):
    f = uniform(0.0, 1.0)(h, w, 'nonfinite')
    f[positions(h, w)[where]] = SPECIALS[special]
    return f


def case_id(name, prm):
    return f'{name}-s{prm[0]:g}-{prm[1]:g}-{prm[2]:g}-c{prm[3]:g}'
