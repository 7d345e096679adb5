"""Input classes of the whole-domain tests of the demosaic and post-processing kernels (tests/test_demosaic_cases.py on the CPU,
tests/test_gpu_demosaic_domain.py on the GPU).  Plain numpy; every frame comes from a seeded generator and depends on
(class, height, width, tile) only, so both files -- and both storage types -- see the same data.

A frame is a control scene with SPARSE special samples.  Where the special samples go is the same for every class (`sites`): a
frame corner, a frame edge, both sides of the vertical and of the horizontal tile seam of the kernel under test, and one sample on
each of the four CFA site classes (row parity, column parity) in the interior.  What goes there is the class:

  scene          the control: nothing special anywhere
  negative       scene - 0.3: many samples below 0, every clamp is live
  ties           flat patches, a block of exact zeros, -0.0, grey pixels (R = G = B: the colour differences are +-0), whole rows of
                 equal samples, a half frame quantised to eighths: gradient comparisons and thresholds sit on equality
  exponents      magnitudes 2^-30 .. 2^30 with 10 % zeros, float32 subnormals (1e-41), a block scaled by 1e-36
  overflow       finite samples up to 3e38: the input is finite, sums and products overflow inside the operator; two blocks of them
                 cover both green phases, so both global green sums overflow
  half_extremes  2^-24, 65504 and values just above 65504, which are infinities in binary16 storage
  nonfinite      isolated NaN, +inf and -inf, a run of four NaNs across the vertical seam; in the RGB form also pixels with two
                 infinite channels of equal sign (inf - inf), a NaN in G alone, an infinite G alone and a 2 x 2 quad of them

The specials stay sparse: tests/test_demosaic_cases.py checks on the oracle alone that at least half of every result is finite.

NAN_REACHES_THE_RESULT: PPG, the colour smoothing, the global equilibration and the white balance end every output in fmaxf(x, 0) (or
a clamp that starts with it), which maps a NaN to 0 -- there a NaN shows as a zero, an infinity or a displaced selection, never as
a NaN.  Bilinear has no clamp, and the local equilibration passes R and B through."""

import zlib

import numpy as np

f32 = np.float32
PATTERNS = ['RGGB', 'BGGR', 'GRBG', 'GBRG']
WORDS = {'RGGB': 0x94949494, 'BGGR': 0x16161616, 'GRBG': 0x61616161, 'GBRG': 0x49494949}
CLASSES = ['scene', 'negative', 'ties', 'exponents', 'overflow', 'half_extremes', 'nonfinite']
NAN_REACHES_THE_RESULT = ('bilinear', 'green_local')
FINITE_CLASSES = ['scene', 'negative', 'ties', 'exponents']   # finite in float32 whatever the operator does with them

# (tile height, tile width) of the kernels, and the frames (h, w) each one runs: the smallest that take each of its paths
# (tests/test_gpu_demosaic_domain.py says which path each frame takes)
TILES = {'bilinear': (16, 128), 'ppg': (32, 64), 'smoothing': (16, 64), 'green_local': (16, 64), 'green_global': (16, 64)}
FRAMES = {'bilinear': [(20, 136), (19, 131), (5, 6)], 'ppg': [(100, 200), (33, 70)], 'smoothing': [(40, 136), (37, 70)],
          'green_local': [(40, 136), (37, 70)], 'green_global': [(40, 136), (37, 70)]}
WB_FRAME = (6, 10)
WB_GAINS = [(0.0, -1.5, 3e38), (3e38, 0.0, -0.25), (-2.0, 3e38, 0.0)]   # 0, a negative value and 3e38 in every slot


def _rng(name, h, w):
    return np.random.default_rng([zlib.crc32(name.encode()), h, w])


def fc_map(h, w, pattern):
    """CFA colour (0 R, 1 G, 2 B) of every site"""
    r, c = np.mgrid[0:h, 0:w]
    return (WORDS[pattern] >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3


def sites(h, w, tile):
    """name -> (row, col) of the special samples.  Frames below 200 pixels carry a corner and an edge sample only: the diamond of a
    third one would leave less than half of a 5 x 6 frame finite."""
    th, tw = tile
    if h * w < 200:
        return {'corner00': (0, 0), 'edge_bottom': (h - 1, w // 2)}
    s = {'corner00': (0, 0), 'corner11': (h - 1, w - 1), 'edge_top': (0, (w // 2) | 1), 'edge_left': ((h // 2) | 1, 0)}
    if w > tw:   # columns tw - 1 | tw are the two sides of the first vertical seam
        s['seam_left'] = (h // 3, tw - 1)
        s['seam_right'] = (h // 3 + 5, tw)
    if h > th:   # rows th - 1 | th of the first horizontal seam
        s['seam_above'] = (th - 1, w // 5)
        s['seam_below'] = (th, w // 5 + 9)
    by, bx = 2 * (h // 8) + 2, 2 * (w // 6) + 2
    dy, dx = 2 * (h // 6) + 1, 2 * (w // 6) + 1   # odd: the four samples sit on the four (row parity, column parity) classes
    s.update({'site00': (by, bx), 'site01': (by, bx + dx), 'site10': (by + dy, bx), 'site11': (by + dy, bx + dx)})
    return s


def seam_run(h, w, tile):
    """four adjacent sites across the first vertical seam (or across the frame's middle column where it has no seam)"""
    x = tile[1] if w > tile[1] else w // 2
    return (2 * h) // 3, slice(x - 2, x + 2)


def scene_rgb(h, w):
    """A smooth colour field with an edge, a dark patch, a patch above 1 and 2 % noise: values in about [-0.05, 1.3]."""
    rng = _rng('scene', h, w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.3 * np.sin(x / 7.0) * np.cos(y / 5.0)
    rgb = np.stack([0.9 * base + 0.1 * x / w, base, 0.7 * base + 0.2 * y / h], -1)
    rgb[h // 3:h // 2, w // 4:w // 2] *= 0.1
    rgb[h // 2:, (3 * w) // 4:] *= 1.4
    return (rgb + rng.normal(0.0, 0.02, rgb.shape)).astype(f32)


def scene_mosaic(h, w):
    """the RGGB mosaic of the scene: one plane, run under all four patterns"""
    return np.take_along_axis(scene_rgb(h, w), fc_map(h, w, 'RGGB')[:, :, None], -1)[:, :, 0].copy()


def _place(a, where, values):
    """values[i % n] at the i-th site; a value is a scalar (every channel) or one entry per channel"""
    for i, (name, pos) in enumerate(where.items()):
        a[pos] = values[i % len(values)]
    return a


def _exponents(a, name, h, w):
    """2^k with k in -30 .. 15 (1 % of the samples: 16 .. 30, which binary16 storage turns into infinities), 10 % zeros, a quarter
    negative; rows h/2 .. h/2 + 3 scaled by 1e-36 (squares and products underflow)."""
    rng = _rng(name, h, w)
    k = np.where(rng.random(a.shape) < 0.01, rng.integers(16, 31, a.shape), rng.integers(-30, 16, a.shape))
    v = np.ldexp(rng.uniform(1.0, 2.0, a.shape), k - 1) * np.where(rng.random(a.shape) < 0.25, -1.0, 1.0)
    v = np.where(rng.random(a.shape) < 0.10, 0.0, v).astype(f32)
    v[h // 2:h // 2 + 4] = (a[h // 2:h // 2 + 4].astype(np.float64) * 1e-36).astype(f32)
    return v


def _apply(name, a, h, w, tile):
    """class `name` on the control frame a: (h, w) or (h, w, 3)"""
    rgb = a.ndim == 3
    where = sites(h, w, tile)
    if name == 'scene':
        return a
    if name == 'negative':
        return (a - f32(0.3)).astype(f32)
    if name == 'ties':
        a[h // 2:] = np.round(a[h // 2:] * f32(8)) / f32(8)           # a half frame on eighths: ties everywhere
        a[2:8, 4:14] = f32(0.25)                                       # a flat patch
        a[h // 4:h // 4 + 6, w // 2:w // 2 + 7] = f32(0.0)             # a block of exact zeros
        a[h // 4 + 2:h // 4 + 4, w // 2 + 2:w // 2 + 5] = f32(-0.0)    # ... with -0.0 inside
        a[h - 5] = f32(0.5)                                            # rows of equal samples
        a[h - 4] = f32(0.5)
        a[h - 3, : w // 2] = f32(0.375)
        if rgb:                                                        # grey pixels: R - G and B - G are +-0
            a[8:14, 2:w - 2] = a[8:14, 2:w - 2, 1:2]
        return _place(a, where, [f32(0.0), f32(-0.0), f32(0.25), f32(0.5)])
    if name == 'exponents':
        v = _exponents(a, name, h, w)
        return _place(v, where, [f32(1e-41), f32(-1e-41), f32(2.0 ** 30), f32(2.0 ** -30), f32(0.0)])
    if name == 'overflow':
        # two 4 x 6 blocks of 2e38 .. 3e38 on even and odd rows and columns: sums of two overflow, and both green phases hold several
        rng = _rng(name, h, w)
        for y0, x0 in ((h // 4, w // 8), ((5 * h) // 8, (5 * w) // 8)) if h * w >= 200 else ():
            blk = a[y0:y0 + 4, x0:x0 + 6]
            blk[...] = rng.uniform(2e38, 3e38, blk.shape).astype(f32)
        return _place(a, where, [f32(3e38), f32(-3e38), f32(1.7e38), f32(3.4e38)])
    if name == 'half_extremes':
        # 65519 rounds to 65504, 65520 and beyond to inf in binary16
        return _place(a, where, [f32(2.0 ** -24), f32(65504.0), f32(65520.0), f32(65519.0), f32(1e5), f32(-65520.0), f32(65536.0)])
    if name == 'nonfinite':
        nan, inf = f32(np.nan), f32(np.inf)
        if rgb:
            vals = [nan, inf, -inf, (inf, inf, 0.3), (0.4, nan, 0.2), (-inf, -inf, -inf), (0.2, inf, 0.7), (inf, 0.5, -inf), (0.3, 0.2, nan)]
        else:
            vals = [nan, inf, -inf]
        _place(a, where, vals)
        if h * w >= 200:
            r, cols = seam_run(h, w, tile)
            a[r, cols] = nan
            if rgb:   # a 2 x 2 quad with G = +inf alone: an infinite green on every site class, so in both green sums of every pattern
                a[h // 2 - 4:h // 2 - 2, w - 12:w - 10, 1] = inf
        return a
    raise KeyError(name)


_cache = {}


def mosaic(name, h, w, tile):
    """float32 (h, w), read-only"""
    key = ('m', name, h, w, tile)
    if key not in _cache:
        a = _apply(name, scene_mosaic(h, w), h, w, tile)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def rgb(name, h, w, tile):
    """float32 (h, w, 3), read-only"""
    key = ('c', name, h, w, tile)
    if key not in _cache:
        a = _apply(name, scene_rgb(h, w), h, w, tile)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def as_stored(a, storage):
    """the frame as the kernel sees it: itself, or its binary16 rounding"""
    if storage == 'f32':
        return a
    with np.errstate(over='ignore'):
        return a.astype(np.float16).astype(f32)


def round_once(ref, storage):
    """the oracle's float32 result as a binary16 store leaves it"""
    return as_stored(ref, storage)


# ---- the frames of the global green equilibration's special ratios
def green_sum_zero(h, w, pattern):
    """every even-row green is 0: sum1 == 0 and the ratio falls back to 1"""
    a = scene_rgb(h, w)
    g1 = (fc_map(h, w, pattern) == 1) & ((np.mgrid[0:h, 0:w][0] & 1) == 0)
    a[:, :, 1] = np.where(g1, f32(0.0), a[:, :, 1])
    return a


def one_nan_green(h, w, pattern, phase):
    """one NaN at a green site of the given row phase: that sum is NaN, `sum > 0` is false, the ratio falls back to 1"""
    a = scene_rgb(h, w)
    ys, xs = np.nonzero((fc_map(h, w, pattern) == 1) & ((np.mgrid[0:h, 0:w][0] & 1) == phase))
    i = len(ys) // 2
    a[ys[i], xs[i], 1] = np.nan
    return a


# ---- what runs: every (operator, configuration, frame) of the GPU module, and the oracle's side of it
def cases():
    """(operator, frame, cfg): cfg holds the pattern and the operator's parameters"""
    out = []
    for frame in FRAMES['bilinear']:
        out += [('bilinear', frame, dict(pattern=p)) for p in PATTERNS]
    for frame in FRAMES['ppg']:
        out += [('ppg', frame, dict(pattern=p, median=m)) for m in (0.0, 1.5) for p in PATTERNS]
    for frame in FRAMES['smoothing']:
        out += [('smoothing', frame, dict(pattern='RGGB', passes=n)) for n in (1, 4, 5)]   # one launch, a full launch, two launches
    for frame in FRAMES['green_local']:
        out += [('green_local', frame, dict(pattern=p, threshold=t)) for t in (0.04, 4.0) for p in PATTERNS]
    for frame in FRAMES['green_global']:
        out += [('green_global', frame, dict(pattern=p)) for p in PATTERNS]
    return out


COMBINED = dict(color_smoothing_passes=5, green_eq_local=True, green_eq_global=True)
COMBINED_CLASSES = ['nonfinite', 'overflow']


def postprocess_args(op, cfg):
    """keyword arguments of PostProcess / oracle.postprocess for a post-processing case"""
    if op == 'smoothing':
        return dict(color_smoothing_passes=cfg['passes'])
    if op == 'green_local':
        return dict(green_eq_local=True, green_eq_threshold=cfg['threshold'])
    if op == 'green_global':
        return dict(green_eq_global=True)
    if op == 'combined':
        return dict(COMBINED)
    raise KeyError(op)


def input_frame(op, name, frame):
    return mosaic(name, *frame, TILES[op]) if op in ('bilinear', 'ppg') else rgb(name, *frame, TILES['smoothing' if op == 'combined' else op])


def run_oracle(oracle, op, cfg, x):
    pat = oracle.PATTERNS[cfg['pattern']]
    if op == 'bilinear':
        return oracle.bilinear5x5(x, pat)
    if op == 'ppg':
        return oracle.ppg(x, pat, cfg['median'])
    return oracle.postprocess(x, pat, **postprocess_args(op, cfg))


def case_id(op, frame, cfg):
    return f'{op}-{frame[0]}x{frame[1]}-' + '-'.join(f'{v:g}' if isinstance(v, float) else str(v) for v in cfg.values())
