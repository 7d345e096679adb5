"""Value classes, frames and footprint arithmetic of the denoiser domain sweep (shared by tests/test_denoise_cases.py, which runs
without a GPU and checks every claim made here against the references alone, and tests/test_gpu_denoise_domain.py).  A plain
helper module: no fixtures, no tests, nothing built or loaded, no GPU code imported.

Footprints.  footprint(p) is the set of result pixels that may change when input sample p changes:

  Wiener    oracle/src/wiener.c: tile origins are the multiples of s = K / ov in (-K, L); a tile READS reflect(o + t), t in
            [0, K) (so a sample within K of a border is also read, mirrored, by tiles that hang over that border) and WRITES
            [o, o + K) cut to the frame.  The footprint is the union of what the reading tiles write; the axes are separable, so
            the 2-D footprint is the product of the 1-D ones.  Away from the borders: [o_min, o_max + K) with o the multiples of
            s in (p - K, p].
            The KERNELS transform two horizontally adjacent tiles (tile columns 2 m and 2 m + 1, counted from the first tile,
            origin -(ov - 1) s) as the real and imaginary part of one complex FFT (csrc/wiener.hip wiener_stream: "z = a + i b";
            csrc/tdk_wiener_ystream.h: "two adjacent tiles ride one complex transform").  Rounding errors of one tile, and a NaN
            or an infinity, therefore reach its partner: the kernels' footprint (pairs=True) is the union of what the reading
            tiles AND their partners write -- up to s columns wider on either side, the same rows.
  NLMeans   nlm_ref of tests/test_gpu_nlmeans.py: Chebyshev radius S + P, cut to the frame (clamped patch reads bring an edge
            sample to patches that are centred within P of it, never further).
  Wavelet   tests/test_wavelet_spec.py: a 5-tap filter at step 2^s per scale, indices clamped: radius 2 (2^scales - 1).
  Bilateral oracle/src/bilateral.c: the sample's own grid cell pair is blurred by two cells either way and read back by the
            pixels whose cell pair meets those six cells: at most BILATERAL_RADIUS[(sigma_s, path)] = 4 sigma_s - 1 pixels either
            way, held against the oracle's changed sets in tests/test_denoise_cases.py.

Value classes of a plane (`classes`): see CLASS_NAMES.  `kind` says what the reference does with a case:
  finite       the reference's result is finite everywhere and is the yardstick;
  nonfinite    a NaN or an infinity: the reference's footprint is non-finite (Wiener), or it states the NaN mask;
  overflowing  finite samples whose squared spectrum overflows float32 in oracle/src/wiener.c (inf / inf = NaN there);
  mixed        scattered_special with every value of SPECIAL14."""

from collections import namedtuple

import numpy as np

INF, NAN = np.float32(np.inf), np.float32(np.nan)
# the list of tests/test_gpu_parity.py::test_bilateral_special_values and test_gpu_lab_chain.py (test_denoise_cases.py reads it back)
SPECIAL14 = np.array([0.0, -0.0, 1e-45, 1e-39, 2.0 ** -41, 2.0 ** -40, 2.0 ** 40, 2.0 ** 41, 1e30, -0.3, -1e30, np.inf, -np.inf, np.nan], np.float32)
SUBNORMALS = np.array([1e-45, -1e-45, 1e-39, -1e-39, 2.0 ** -127, 1.1754942e-38], np.float32)   # the last: the largest subnormal
F16_EXTREMES = np.array([65504.0, -65504.0, 6e-8, -0.0], np.float32)
FLAT_VALUES = [0.0, -0.0, 1e-30, -5.0, 65504.0, 1e10]
SCALES = [1e-3, 1e3, 1e6]
HUGE = [1e18, -1e18]
OVERFLOWING = [1e30, 3e38]
SINGLE = {'single_nan': [NAN], 'single_pinf': [INF], 'single_ninf': [-INF], 'single_huge': HUGE, 'single_overflowing': OVERFLOWING}
CLASS_NAMES = ['negative', 'scaled', 'flat', 'subnormal', 'f16_extremes', 'single_nan', 'single_pinf', 'single_ninf', 'single_huge',
               'single_overflowing', 'scattered_special']
SHARE = 0.01   # scattered classes: about this share of the pixels

# Wiener frames (W, H): the smallest entries of wc.STRIP_SHAPES / wc.GROUP_SHAPES with 3 x 3 workgroups (an interior one, edge
# ones, a partial last strip / group and a partial last segment / band), and the group geometry (tile columns, tile rows) there
WIENER_FRAMES = {(32, 4): (361, 105), (16, 4): (56, 117), (32, 2): (256, 241)}
# the strip kernel's interior body needs W % 4 == 0 and a workgroup clear of every edge (include/tdk_hip_wiener.h: 1 <= strip <
# W / 128, 1 <= segment < H / 64), which no table entry has: the smallest such frame with a partial last strip and segment, for
# the samples inside that workgroup (strip 1 = columns 104 .. 255, segment 1 = rows 40 .. 127)
WIENER_INTERIOR_FRAME = (392, 193)
WIENER_INTERIOR_POSITIONS = {'interior-body': (85, 170), 'interior-body-seam': (104, 232)}
WIENER_GROUP = {(32, 4): (16, 8), (16, 4): (8, 16), (32, 2): (8, 8)}
BILATERAL_PATHS = {'tiles': (2.0, 0.2), 'grid': (8.0, 0.1)}
BILATERAL_RADIUS = {(2.0, 'tiles'): 7, (8.0, 'grid'): 31}   # 4 sigma_s - 1: the changed set lies in the box of (2 R + 1)^2, cut to the frame
LAB_LIPSCHITZ = 8.0   # |d (L, a, b)| <= this * sum |d rgb_c| on [0, 1]^3 (test_denoise_cases.py measures 4.5)
BILATERAL_SHAPES = [(96, 128), (61, 99)]   # (h, w): W % 4 == 0 (vector loads) and W % 4 == 3
NLM_SHAPE, NLM_S, NLM_P = (37, 53), 3, 1
WAVELET_SHAPE = (75, 83)

Case = namedtuple('Case', 'name frame clean sigma_scale samples kind')   # samples: [(y, x, value)]; clean: the frame without them


# ---------------------------------------------------------------------------------------------------------------- footprints
def _reflect(x, limit):
    x = np.where(x < 0, -x, x)
    return np.where(x >= limit, 2 * limit - x - 1, x)


def _tile_reads(p, L, K, ov):
    """(origins, how often each tile reads sample p): 0, 1, or 2 for a tile that also reads it mirrored at a frame edge."""
    s = K // ov
    origins = [j * s for j in range(-(ov - 1), (L - 1) // s + 1)]   # every multiple of s with o + K > 0 and o < L
    return origins, [int((_reflect(o + np.arange(K), L) == p).sum()) for o in origins]


def _written(origins, flags, L, K, pairs):
    if pairs:
        flags = [f or (t ^ 1 < len(flags) and flags[t ^ 1]) for t, f in enumerate(flags)]
    mask = np.zeros(L, bool)
    for o, f in zip(origins, flags):
        if f:
            mask[max(o, 0):min(o + K, L)] = True
    return mask


def wiener_footprint(p, L, K, ov, pairs=False):
    """Boolean mask over [0, L): the result samples that tiles reading input sample p write (pairs: and their FFT partners)."""
    origins, reads = _tile_reads(p, L, K, ov)
    return _written(origins, [r > 0 for r in reads], L, K, pairs)


def wiener_footprint2d(y, x, H, W, K, ov, pairs=False):
    """(H, W) mask; only horizontally adjacent tiles share a transform, so `pairs` widens the columns alone."""
    return np.outer(wiener_footprint(y, H, K, ov), wiener_footprint(x, W, K, ov, pairs))


def wiener_sum_overflow2d(y, x, v, H, W, K, ov):
    """(H, W) mask of what the KERNELS' tiles (and FFT partners) write whose float32 sample sum overflows because they read the
    sample v at (y, x) ny * nx times, mirrored reads included, with ny * nx * |v| above FLT_MAX (every other sample is of order
    one): for v = 3e38, the tiles that read it at least twice.  Empty for 1e30 and away from the frame's edges."""
    need = float(np.finfo(np.float32).max) / abs(float(v))
    oy, ry = _tile_reads(y, H, K, ov)
    ox, rx = _tile_reads(x, W, K, ov)
    out = np.zeros((H, W), bool)
    for ny in sorted(set(ry) - {0}):
        cols = _written(ox, [nx > 0 and ny * nx > need for nx in rx], W, K, True)
        out |= np.outer(_written(oy, [r == ny for r in ry], H, K, False), cols)
    return out


def box_footprint2d(y, x, H, W, radius):
    m = np.zeros((H, W), bool)
    m[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1] = True
    return m


def nlm_footprint2d(y, x, H, W, S, P):
    return box_footprint2d(y, x, H, W, S + P)


def wavelet_radius(scales):
    return 2 * ((1 << scales) - 1)


def wavelet_footprint2d(y, x, H, W, scales):
    return box_footprint2d(y, x, H, W, wavelet_radius(scales))


def bilateral_footprint2d(y, x, H, W, sigma_s, path):
    return box_footprint2d(y, x, H, W, BILATERAL_RADIUS[(sigma_s, path)])


def union(masks, shape):
    out = np.zeros(shape, bool)
    for m in masks:
        out |= m
    return out


def wiener_scale(case, K, ov, pairs=True):
    """Per pixel: max(1, the largest |input| among the tiles -- with `pairs`, the tile pairs -- that cover it).  The frame without
    its samples counts with its maximum (it is of one order of magnitude throughout); every sample raises its own footprint."""
    H, W = case.frame.shape
    scale = np.full((H, W), max(1.0, float(np.abs(case.clean).max())))
    for y, x, v in case.samples:
        if np.isfinite(v):
            m = wiener_footprint2d(y, x, H, W, K, ov, pairs)
            scale[m] = np.maximum(scale[m], abs(float(v)))
    return scale


# ---------------------------------------------------------------------------------------------------------------- positions
def sample_positions(h, w, seam=None):
    """{name: (y, x)}: inside the frame's interior, next to each border (within any K, S + P or filter radius of it), both
    corners -- the bottom right one lies in the last partial strip / group and segment / band -- and `seam` if given."""
    pos = {'interior': (h // 2 + 1, w // 2 + 3), 'top': (2, w // 3), 'bottom': (h - 3, 2 * w // 3), 'left': (h // 3, 1),
           'right': (2 * h // 3, w - 2), 'corner00': (0, 0), 'corner11': (h - 1, w - 1)}
    if seam is not None:
        pos['seam'] = seam
    return pos


def wiener_seam(K, ov):
    """(y, x) of the first sample of the second group row / column: the first row (column) of the first tile of band (strip /
    group) 1, which is also covered by the last ov - 1 tiles of band 0 -- both sides of the seam write it."""
    G, TR = WIENER_GROUP[(K, ov)]
    s = K // ov
    return ((TR - (ov - 1)) * s, (G - (ov - 1)) * s)


def wiener_positions(K, ov):
    w, h = WIENER_FRAMES[(K, ov)]
    return sample_positions(h, w, wiener_seam(K, ov))


# ---------------------------------------------------------------------------------------------------------------- classes
def _scatter(base, values, seed, share=SHARE):
    """base with about `share` of its samples replaced by draws from `values`; returns (frame, [(y, x, value)])."""
    rng = np.random.default_rng(seed)
    h, w = base.shape
    n = max(int(round(share * h * w)), len(values))
    flat = rng.choice(h * w, n, replace=False)
    vals = np.asarray(values, np.float32)[np.arange(n) % len(values)]   # every value occurs
    out = base.copy()
    out.flat[flat] = vals
    return out, [(int(i // w), int(i % w), np.float32(v)) for i, v in zip(flat, vals)]


def classes(base, positions, only=None):
    """Every case of every class on the float32 plane `base` (a scene channel, in [0, 1]).  positions: {name: (y, x)} for the
    single_* classes; `only`: an iterable of class names."""
    base = np.ascontiguousarray(base, np.float32)
    assert base.ndim == 2 and base.min() >= 0.0 and base.max() <= 1.0
    want = set(only or CLASS_NAMES)
    assert want <= set(CLASS_NAMES), want
    out = []

    def add(name, frame, kind, sigma_scale=1.0, samples=(), clean=None):
        frame = np.ascontiguousarray(frame, np.float32)
        out.append(Case(name, frame, frame if clean is None else clean, sigma_scale, list(samples), kind))

    if 'negative' in want:
        add('negative', base * np.float32(7.0) - np.float32(3.0), 'finite')
    if 'scaled' in want:
        for s in SCALES:
            add(f'scaled[{s:g}]', base * np.float32(s), 'finite', s)
    if 'flat' in want:
        for c in FLAT_VALUES:
            add(f'flat[{c!r}]', np.full(base.shape, c, np.float32), 'finite')
    if 'subnormal' in want:
        f, smp = _scatter(base, SUBNORMALS, 3)
        add('subnormal', f, 'finite', samples=smp, clean=base)
    if 'f16_extremes' in want:
        f, smp = _scatter(base, F16_EXTREMES, 4)
        add('f16_extremes', f, 'finite', samples=smp, clean=base)
    for name, values in SINGLE.items():
        if name not in want:
            continue
        kind = {'single_huge': 'finite', 'single_overflowing': 'overflowing'}.get(name, 'nonfinite')
        for pname, (y, x) in positions.items():
            for v in values:
                f = base.copy()
                f[y, x] = v
                add(f'{name}[{float(v):g}@{pname}]', f, kind, samples=[(y, x, np.float32(v))], clean=base)
    if 'scattered_special' in want:
        f, smp = _scatter(base, SPECIAL14, 5)
        tame = f.copy()
        keep = []
        for y, x, v in smp:   # the same places; the values oracle/src/wiener.c cannot digest give way to the scene's
            if is_tame(v):
                keep.append((y, x, v))
            else:
                tame[y, x] = base[y, x]
        add('scattered_special[tame]', tame, 'finite', samples=keep, clean=base)   # before [all], which is compared with it
        add('scattered_special[all]', f, 'mixed', samples=smp, clean=base)
    return out


def is_tame(v):
    """Finite, and small enough that its squared spectrum stays finite in float32 (|v| <= 2^41 < 1.8e19)."""
    return bool(np.isfinite(v)) and abs(float(v)) <= 2.0 ** 41


def as_f16(case):
    """The case as binary16 storage sees it (values rounded once), or None where that changes the class: a finite sample that
    becomes infinite (1e18, 1e6 x scene, 1e10, the 2^40 of the tame scattered frame), or subnormals / 1e-30 that become zero.
    scattered_special[all] is a mixed case before and after: its 2^40, 2^41 and 1e30 arrive as infinities."""
    with np.errstate(over='ignore'):
        r = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
        frame, clean = r(case.frame), r(case.clean)
    if case.kind != 'mixed' and (not np.array_equal(np.isfinite(frame), np.isfinite(case.frame)) or case.name in ('subnormal', 'flat[1e-30]')):
        return None
    samples = [(y, x, frame[y, x]) for y, x, _ in case.samples]
    return case._replace(frame=frame, clean=clean, samples=samples)


def rgb_case(case, rgb, channel=1):
    """A (H, W, 3) version for the interleaved kernels: the scene's other two channels take the same affine map as the plane
    (scaled / negative / flat) and stay clean otherwise; the samples sit in `channel`."""
    frame = np.repeat(case.frame[:, :, None], 3, 2) if not case.samples and case.name.startswith('flat') else None
    if frame is None:
        others = np.ascontiguousarray(rgb, np.float32).copy()
        if case.name == 'negative':
            others = others * np.float32(7.0) - np.float32(3.0)
        elif case.name.startswith('scaled'):
            others = others * np.float32(case.sigma_scale)
        frame = others
        frame[:, :, channel] = case.frame
    return np.ascontiguousarray(frame)


# ---------------------------------------------------------------------------------------------------------------- RGB pixels
def special_rgb_frame(scene_rgb, pixels, seed=6, share=SHARE):
    """The scene with about `share` of its pixels replaced by rows of `pixels` ((N, 3): color_domain_spec.special_pixels()), every
    row at least once.  Returns (frame, mask (H, W) of the replaced pixels, index (H, W) of the row placed, -1 elsewhere)."""
    rng = np.random.default_rng(seed)
    h, w, _ = scene_rgb.shape
    n = max(int(round(share * h * w)), len(pixels))
    flat = rng.choice(h * w, n, replace=False)
    idx = np.full(h * w, -1)
    idx[flat] = np.arange(n) % len(pixels)
    idx = idx.reshape(h, w)
    out = np.ascontiguousarray(scene_rgb, np.float32).copy()
    out[idx >= 0] = np.asarray(pixels, np.float32)[idx[idx >= 0]]
    return out, idx >= 0, idx
