"""NaN-faithful float64 NumPy specification of the colour operators, luminance extract / replace, normalize_image and the four
tone mappers, valid for EVERY float input (negative, zero, above the clip, infinite, NaN), with a per-value sensitivity.

tests/test_second_source_color.py restates the same formulas for in-gamut pixels; outside [0, 1] that restatement is not a
specification (its `powp` clamps a negative base, np.clip propagates NaN).  Here the semantics are those of the reference's C:
  * pow of a negative base (non-integer exponent) is NaN, pow(x, 0) is 1 for every x;
  * every fmaxf / fminf / clip DROPS a NaN operand (np.fmax / np.fmin), so clip(NaN) == 0;
  * every comparison is written as in oracle/src/color.h and color_ops.c (`>` against `<=`, `t3 > 0.008856`, `delta > 1e-6`,
    `s < 1e-6`) and is false on NaN; the hue wheel's sequential `if`s become nested `np.where`s in the same order;
  * literals are the float32 values the C source names (`0.04045f`), evaluated in float64, so that a pixel ON a branch
    constant takes the same branch in both.
Nothing here is shared with the kernels or the oracle.

Sensitivity.  A float32 implementation cannot do better than the condition of the function allows: `s_i` is the largest change
of the float64 result of value i when ONE input channel moves by +-(|x| * 2^-21 + 2^-24), over the channels and both signs.  A
value is held to `(A + K * s_i) * scale` with `scale = max(1, largest pre-clip intermediate of the pixel)`: its inputs, pre-clip
outputs and the linear-light / XYZ values in between (an over-range pixel goes through the Lab round trip at that magnitude, and
fp32 rounding is relative to it).  The scale multiplies A as well: the dark channel of such a pixel comes out of a cancelling
3x3 product whose rounding error is relative to the LARGE operands, while the result does not move with the inputs at all
(s_i ~ 1e-11), so `A + K * s_i * scale` could not hold the fp32 oracle there for any K below 2^20.  Where the operator clips and
the pre-clip value lies further than the bound outside [0, 1], the bound is 0: the result must be exactly 0 or 1.  A perturbed result that becomes NaN where
the unperturbed one is not (or the reverse) has infinite sensitivity.

CONSTANTS holds (A_op, K_op) per operator: the smallest powers of two at which the fp32 C oracle meets the bound on every
non-excluded value of every case of tests/test_color_domain_spec.py -- found by `python tests/color_domain_spec.py` with the rule
"among the minimal passing pairs (no passing pair has both a smaller A and a smaller K; A <= 2^-16, 0.004 uint8 steps) the one
that excludes the fewest values, then the smaller K, then the smaller A".  The GPU kernels are held to 8x that
bound (tests/test_gpu_color_domain.py).  A value is EXCLUDED (ill-conditioned in the reference itself) only when its GPU bound
exceeds EXCLUDE = 1e-3, a quarter of a uint8 step; both test files assert that this is at most 1 % of a case.
float32 denormal inputs are outside the tested domain (the hardware log / exp flush them; no stage of the chain produces them).
"""

import functools

import numpy as np

EXCLUDE = 1e-3      # a GPU bound above this marks an ill-conditioned value
EXCLUDE_CAP = 0.01  # at most this share of a case may be excluded
A_MAX = 2.0 ** -16  # the largest absolute term the rule below may choose
GPU_FACTOR = 8.0    # v_log_f32 / v_exp_f32 / v_rcp_f32 are ~1 ulp each, exp2(y log2 x) multiplies the log's error by |y log2 x|


def c32(v):
    """The float32 literal `v`f as a float64."""
    return float(np.float32(v))


M_RGB2XYZ = np.array([[c32(v) for v in r] for r in
                      [[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]]])
M_XYZ2RGB = np.array([[c32(v) for v in r] for r in
                      [[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]]])
D65 = np.array([c32(0.95047), 1.0, c32(1.08883)])


def _quiet(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with np.errstate(all='ignore'):
            return fn(*a, **k)
    return wrapped


def cpow(x, y):
    """C pow: NaN for a negative base and a non-integer exponent, 1 for y == 0 whatever x is."""
    return np.power(x, y)


def clip01(x):
    """fminf(fmaxf(x, 0), 1): a NaN becomes 0."""
    return np.fmin(np.fmax(x, 0), 1.0)


_PROBE = None  # while evaluate() runs: the per-pixel magnitudes of every 3x3 product's operands (linear light, XYZ, ACES)


def _finite_max(*arrays):
    m = np.concatenate([np.abs(a).reshape(a.shape[0], -1) for a in arrays], 1)
    return np.where(np.isfinite(m), m, 0.0).max(1, keepdims=True)


def mat(m, v):
    """row-major 3x3 times vector, summed left to right as the C does (matters only for inf - inf)."""
    r = np.stack([m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1] + m[r, 2] * v[:, 2] for r in range(3)], -1)
    if _PROBE is not None:
        _PROBE.append(_finite_max(v, r))
    return r


# ---------------------------------------------------------------- header A (oracle/src/color.h cA_*)
class A:
    T_SRGB, T_LIN, T_LAB = c32(0.04045), c32(0.0031308), c32(0.008856)
    K_LAB, OFF = c32(7.787), c32(16.0 / 116.0)

    @classmethod
    def srgb_to_linear(cls, c):
        a = c32(0.055)
        return np.where(c > cls.T_SRGB, cpow((c + a) / c32(1.055), c32(2.4)), c * c32(1.0 / 12.92))

    @classmethod
    def linear_to_srgb(cls, c):
        a = c32(0.055)
        return np.where(c > cls.T_LIN, c32(1.055) * cpow(c, c32(1.0 / 2.4)) - a, c * c32(12.92))

    @classmethod
    def lab_f(cls, t):
        return np.where(t > cls.T_LAB, cpow(t, c32(1.0 / 3.0)), t * cls.K_LAB + cls.OFF)

    @classmethod
    def lab_f_inv(cls, t):
        t3 = t * t * t
        return np.where(t3 > cls.T_LAB, t3, (t - cls.OFF) / cls.K_LAB)

    @classmethod
    def rgb_to_xyz(cls, rgb):
        return mat(M_RGB2XYZ, cls.srgb_to_linear(rgb))

    @classmethod
    def xyz_to_lab(cls, xyz):
        f = cls.lab_f(xyz / D65)
        return np.stack([c32(116.0 / 100.0) * f[:, 1] - c32(16.0 / 100.0), c32(500.0 / 128.0) * (f[:, 0] - f[:, 1]),
                         c32(200.0 / 128.0) * (f[:, 1] - f[:, 2])], -1)

    @classmethod
    def lab_to_xyz(cls, lab):
        fy = lab[:, 0] * c32(100.0 / 116.0) + cls.OFF
        f = np.stack([lab[:, 1] * c32(128.0 / 500.0) + fy, fy, fy - lab[:, 2] * c32(128.0 / 200.0)], -1)
        return cls.lab_f_inv(f) * D65

    @classmethod
    def xyz_to_rgb(cls, xyz):
        return cls.linear_to_srgb(mat(M_XYZ2RGB, xyz))

    @classmethod
    def rgb_to_lab(cls, rgb):
        return cls.xyz_to_lab(cls.rgb_to_xyz(rgb))

    @classmethod
    def lab_to_rgb(cls, lab):
        return cls.xyz_to_rgb(cls.lab_to_xyz(lab))

    @classmethod
    def lab_l(cls, rgb):
        lin = cls.srgb_to_linear(rgb)
        y = M_RGB2XYZ[1, 0] * lin[:, 0] + M_RGB2XYZ[1, 1] * lin[:, 1] + M_RGB2XYZ[1, 2] * lin[:, 2]
        return np.fmax(0.0, c32(116.0 / 100.0) * cls.lab_f(y) - c32(16.0 / 100.0))

    @classmethod
    def replace_l(cls, rgb, new_l):
        lab = cls.rgb_to_lab(rgb)
        return cls.lab_to_rgb(np.stack([np.fmax(0.0, np.fmin(1.0, new_l)), lab[:, 1], lab[:, 2]], -1))

    @classmethod
    def vibrance_preclip(cls, rgb, amount):
        lab = cls.rgb_to_lab(rgb)
        chroma = np.sqrt(lab[:, 1] * lab[:, 1] + lab[:, 2] * lab[:, 2])
        ls, ss = 1.0 - amount * chroma * 0.25, 1.0 + amount * chroma
        return cls.lab_to_rgb(np.stack([lab[:, 0] * ls, lab[:, 1] * ss, lab[:, 2] * ss], -1))

    @staticmethod
    def rgb_to_hsl(rgb):
        r, g, b = rgb.T
        mx, mn = np.fmax(np.fmax(r, g), b), np.fmin(np.fmin(r, g), b)
        d = mx - mn
        l = (mx + mn) * 0.5
        ok = d > c32(1e-6)
        s = np.where(l < 0.5, d / (mx + mn), d / (2.0 - mx - mn))
        h = np.where(mx == r, (g - b) / d + np.where(g < b, 6.0, 0), np.where(mx == g, (b - r) / d + 2.0, (r - g) / d + 4.0)) / 6.0
        return np.stack([np.where(ok, h, 0), np.where(ok, s, 0), l], -1)

    @staticmethod
    def hue(p, q, t):
        t = np.where(t < 0.0, t + 1.0, t)
        t = np.where(t > 1.0, t - 1.0, t)
        return np.where(t < c32(1.0 / 6.0), p + (q - p) * 6.0 * t,
                        np.where(t < 0.5, q, np.where(t < c32(2.0 / 3.0), p + (q - p) * (c32(2.0 / 3.0) - t) * 6.0, p)))

    @classmethod
    def hsl_to_rgb(cls, hsl):
        h, s, l = hsl.T
        q = np.where(l < 0.5, l * (1.0 + s), l + s - l * s)
        p = 2.0 * l - q
        third = c32(1.0 / 3.0)
        rgb = np.stack([cls.hue(p, q, h + third), cls.hue(p, q, h), cls.hue(p, q, h - third)], -1)
        return np.where((s < c32(1e-6))[:, None], l[:, None], rgb)

    @classmethod
    def modify_hsl_preclip(cls, rgb, dh, ds, dl):
        dh, ds, dl = c32(dh), c32(ds), c32(dl)
        hsl = cls.rgb_to_hsl(rgb)
        h = hsl[:, 0] + dh
        h = np.where(h < 0.0, h + 1.0, h)
        h = np.where(h > 1.0, h - 1.0, h)
        return cls.hsl_to_rgb(np.stack([h, cpow(hsl[:, 1], 1.0 / (1.0 + ds)), cpow(hsl[:, 2], 1.0 / (1.0 + dl))], -1))


# ---------------------------------------------------------------- header B (oracle/src/color.h cB_*)
class B:
    DELTA = c32(6.0 / 29.0)
    DELTA3 = c32(c32(DELTA * DELTA) * DELTA)           # delta * delta * delta, evaluated in float32
    FACTOR_INV = c32(3.0 * c32(DELTA * DELTA))         # 3 * delta * delta
    FACTOR = c32(1.0 / FACTOR_INV)
    OFF = c32(4.0 / 29.0)

    @staticmethod
    def srgb_to_linear(c):
        return np.where(c <= c32(0.04045), c / c32(12.92), cpow((c + c32(0.055)) / c32(1.055), c32(2.4)))

    @staticmethod
    def linear_to_srgb(c):
        return np.where(c <= c32(0.0031308), c32(12.92) * c, c32(1.055) * cpow(c, c32(1.0 / 2.4)) - c32(0.055))

    @classmethod
    def rgb_to_lab(cls, rgb):
        n = mat(M_RGB2XYZ, cls.srgb_to_linear(rgb)) / D65
        f = np.where(n > cls.DELTA3, np.cbrt(n), cls.FACTOR * n + cls.OFF)
        return np.stack([(116.0 * f[:, 1] - 16.0) / 100.0, 500.0 * (f[:, 0] - f[:, 1]) / 128.0, 200.0 * (f[:, 1] - f[:, 2]) / 128.0], -1)

    @classmethod
    def lab_to_rgb(cls, lab):
        fy = (lab[:, 0] * 100.0 + 16.0) / 116.0
        f = np.stack([lab[:, 1] * 128.0 / 500.0 + fy, fy, fy - lab[:, 2] * 128.0 / 200.0], -1)
        xyz = np.where(f > cls.DELTA, f * f * f, cls.FACTOR_INV * (f - cls.OFF)) * D65
        return cls.linear_to_srgb(mat(M_XYZ2RGB, xyz))

    @classmethod
    def vibrance_preclip(cls, rgb, amount):
        lab = cls.rgb_to_lab(rgb)
        chroma = np.sqrt(lab[:, 1] * lab[:, 1] + lab[:, 2] * lab[:, 2])
        ls, ss = 1.0 - amount * chroma * 0.25, 1.0 + amount * chroma
        return cls.lab_to_rgb(np.stack([lab[:, 0] * ls, lab[:, 1] * ss, lab[:, 2] * ss], -1))


# ---------------------------------------------------------------- tone mappers (oracle/src/color_ops.c tonemap_pixel)
ACES_IN = np.array([[c32(v) for v in r] for r in [[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]]])
ACES_OUT = np.array([[c32(v) for v in r] for r in [[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]]])


def map_key(log_mean):
    n = np.fmax(0.0, np.fmin(1.0, (-log_mean) / c32(9.21034)))
    return c32(0.3) + c32(0.7) * cpow(n, c32(1.4))


def aces_fit(rgb):
    v = mat(ACES_IN, rgb)
    a = v * (v + c32(0.0245786)) - c32(0.000090537)
    b = v * (c32(0.983729) * v + c32(0.4329510)) + c32(0.238081)
    return mat(ACES_OUT, a / b)


def tonemap_preclip(name, rgb, metrics, gamma, intensity, light_adapt, vibrance):
    """(pre-clip output of the vibrance stage, the gamma-encoded value g that enters it)."""
    gamma, intensity, light_adapt, vibrance = (float(np.float32(v)) for v in (gamma, intensity, light_adapt, vibrance))
    metrics = np.asarray(metrics, np.float32).astype(np.float64)
    if name == 'aces':
        tm = aces_fit(rgb * cpow(2.0, intensity))
    else:
        mean = metrics[2:5][None] + light_adapt * (rgb - metrics[2:5][None])
        adapt = cpow(mean / np.exp(intensity), map_key(metrics[0]))
        if name == 'reinhard':
            tm = rgb / (adapt + rgb)
        elif name == 'linear':
            tm = rgb / adapt
        else:
            tm = aces_fit(rgb / adapt)
    ig = float(np.float32(1.0) / np.float32(gamma))
    g = cpow(np.fmax(tm, 0), ig)
    return B.vibrance_preclip(g, vibrance), g


# ---------------------------------------------------------------- the operators under test, as functions of an (N, C) input
def _evaluate(op, x, p):
    """(pre-clip result, clips to [0, 1]?, further intermediates for the scale)"""
    rgb = x[:, :3]
    if op in ('rgb_to_xyz', 'xyz_to_lab', 'lab_to_xyz', 'xyz_to_rgb', 'rgb_to_lab', 'lab_to_rgb'):
        return getattr(A, op)(rgb), False, rgb
    if op == 'modify_hsl':
        return A.modify_hsl_preclip(rgb, *p), True, rgb
    if op == 'modify_vibrance':
        return A.vibrance_preclip(rgb, c32(p[0])), True, rgb
    if op in ('compute_luminance', 'compute_log_luminance'):
        lum = A.lab_l(clip01(rgb))
        r = np.log(np.fmax(c32(p[0]), lum)) if op == 'compute_log_luminance' else lum
        return r[:, None], False, r[:, None] * 0.0
    if op in ('modify_luminance', 'modify_log_luminance'):
        new_l = np.exp(x[:, 3]) if op == 'modify_log_luminance' else x[:, 3]
        return A.replace_l(rgb, new_l), True, rgb
    if op == 'normalize_image':
        b0, b1 = c32(p[0]), c32(p[1])
        return (x - b0) / (b1 - b0), False, x
    if op.startswith('tonemap_'):
        r, g = tonemap_preclip(op[len('tonemap_'):], rgb, *p)
        return r, True, g
    raise KeyError(op)


@_quiet
def evaluate(op, x, params=None, probe=False):
    """x: (N, C) float64 (C = 3, or 4 with the luminance plane last for the replace ops).  Returns (result (N, M), pre-clip
    result or None, scale (N, 1) or None); the result is what the operator returns (after its clip, if it has one).
    scale (with `probe`) = max(1, the largest finite magnitude among the pixel's inputs, pre-clip outputs and the operands of
    every 3x3 product on the way: linear light, XYZ)."""
    global _PROBE
    _PROBE = [] if probe else None
    try:
        pre, clips, extra = _evaluate(op, x, params or ())
        scale = np.fmax(1.0, np.concatenate(_PROBE + [_finite_max(pre, extra)], 1).max(1, keepdims=True)) if probe else None
    finally:
        _PROBE = None
    return (clip01(pre), pre, scale) if clips else (pre, None, scale)


def _absdiff(a, b):
    """|a - b| with inf - inf (same sign) and NaN - NaN counted as 0, NaN against a number as inf."""
    with np.errstate(all='ignore'):
        d = np.abs(a - b)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return np.where(same, 0.0, np.where(np.isnan(d), np.inf, d))


def evaluate_with_sensitivity(op, x32, params=None):
    """x32: (N, C) float32 input as the kernel sees it.  Returns (result, sensitivity, scale, pre-clip result or None), float64."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    base, pre, scale = evaluate(op, x, params, probe=True)
    sens = np.zeros_like(base)
    for c in range(x.shape[1]):
        step = np.abs(x[:, c]) * 2.0 ** -21 + 2.0 ** -24
        step = np.where(np.isfinite(step), step, 0.0)
        for sign in (1.0, -1.0):
            xp = x.copy()
            xp[:, c] += sign * step
            sens = np.fmax(sens, _absdiff(evaluate(op, xp, params)[0], base))
    return base, sens, scale, pre


def bound(op_key, sens, scale, pre=None, factor=1.0, ak=None):
    """factor * (A + K * s_i) * scale; 0 where the operator clips and the pre-clip value is further than that outside [0, 1]
    (clipping is 1-Lipschitz and saturates: whatever lies within the bound of such a value clips to exactly 0 or 1)."""
    a, k = ak or CONSTANTS[op_key][:2]
    with np.errstate(all='ignore'):
        b = factor * (a + k * sens) * scale
        if pre is not None:
            b = np.where((pre - b >= 1.0) | (pre + b <= 0.0), 0.0, b)
    return b


def excluded(op_key, sens, scale, pre=None, ak=None):
    return ~(bound(op_key, sens, scale, pre, GPU_FACTOR, ak) <= EXCLUDE)


def quantise(v):
    """uint8 of a clipped value: round(clip(v) * 255), half away from zero (the value is non-negative)."""
    return np.floor(clip01(v) * 255.0 + 0.5)


def tie_distance(v):
    """distance of clip(v) * 255 from the nearest rounding tie n + 0.5."""
    t = clip01(v) * 255.0
    return np.abs(t - np.floor(t) - 0.5)


# ---------------------------------------------------------------- pixel sets
def _around(k, steps):
    """float32 values `steps` ulps around the float32 constant k."""
    k = np.float32(k)
    out = []
    for s in steps:
        v = k
        for _ in range(abs(s)):
            v = np.nextafter(v, np.float32(np.inf if s > 0 else -np.inf), dtype=np.float32)
        out.append(v)
    return np.array(out, np.float32)


STEPS = (-3, -2, -1, 0, 1, 2, 3)


def _branch_rgb(rng):
    """RGB pixels on both sides of every branch of the RGB-input operators."""
    px = []
    # sRGB decode thresholds on the input itself, each in every channel position, the other channels random
    for k in (0.04045, 0.0031308, 0.0, 1.0, 0.5):
        for v in _around(k, STEPS):
            for ch in range(3):
                p = rng.uniform(0.0, 1.0, 3).astype(np.float32)
                p[ch] = v
                px.append(p)
            px.append(np.full(3, v, np.float32))
    # lab_f thresholds on Y (and on X / Xn, Z / Zn for a grey): greys whose linear value sits within +-2e-6 of the constant
    for t in (0.008856, (6.0 / 29.0) ** 3):
        c = 1.055 * t ** (1 / 2.4) - 0.055
        for v in c + rng.uniform(-2e-6, 2e-6, 24):
            px.append(np.full(3, v, np.float32))
    # HSL: delta around 1e-6, l around 0.5 (mx + mn around 1), s < 1e-6, the six hue sector borders (two channels equal or a few ulps apart)
    for base in (0.2, 0.5, 0.8):
        for d in _around(1e-6, STEPS) * 1.0:
            px.append(np.array([base + d, base, base], np.float32))
            px.append(np.array([base, base, base + d], np.float32))
    for mx in (0.6, 0.75, 0.9):
        for v in _around(1.0 - mx, STEPS):
            px.append(np.array([mx, v, rng.uniform(v, mx)], np.float32))
    for hi, lo in ((0.7, 0.2), (0.9, 0.4), (0.35, 0.05)):
        for v in _around(hi, STEPS):
            px += [np.array(p, np.float32) for p in ((hi, v, lo), (v, hi, lo), (lo, hi, v), (lo, v, hi), (v, lo, hi), (hi, lo, v))]
        for v in _around(lo, STEPS):
            px += [np.array(p, np.float32) for p in ((hi, v, lo), (v, hi, lo), (lo, hi, v), (lo, v, hi), (v, lo, hi), (hi, lo, v))]
    return np.array(px, np.float32)


def _branch_xyz(rng):
    px = []
    for t in (0.008856, (6.0 / 29.0) ** 3, 0.0031308, 0.0):
        for v in _around(t, STEPS):
            for ch in range(3):
                p = rng.uniform(0.0, 1.0, 3).astype(np.float32)
                p[ch] = np.float32(v * D65[ch])
                px.append(p)
            px.append((v * D65).astype(np.float32))
    return np.array(px, np.float32)


def _branch_lab(rng):
    px = []
    for f in (0.008856 ** (1 / 3), 6.0 / 29.0):
        l0 = (f - 16.0 / 116.0) * 1.16
        for v in l0 + rng.uniform(-2e-6, 2e-6, 24):
            px.append(np.array([v, 0.0, 0.0], np.float32))
            px.append(np.array([v, rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)], np.float32))
            px.append(np.array([rng.uniform(0.2, 0.9), 0.0, 0.0], np.float32))
    return np.array(px, np.float32)


N_PIXELS = 19999  # 4 k + 3: vector body and a three-pixel tail; the first N - 3 / N - 2 pixels give 4 k / 4 k + 1


@functools.lru_cache(maxsize=None)
def pixels(kind):
    """(N_PIXELS, 3) float32, shuffled so that every prefix holds every set.  kind: 'rgb', 'xyz' or 'lab'."""
    rng = np.random.default_rng({'rgb': 101, 'xyz': 102, 'lab': 103}[kind])
    if kind == 'lab':
        lab = rng.uniform(-0.8, 0.8, (12000, 3))
        lab[:, 0] = rng.uniform(-0.3, 1.4, 12000)   # L outside [0, 1] too
        grey = np.zeros((2000, 3))
        grey[:, 0] = rng.uniform(-0.3, 1.4, 2000)
        parts = [lab, grey, _branch_lab(rng)]
    else:
        grey = np.repeat(rng.uniform(-0.25, 1.6, (2000, 1)), 3, 1)
        parts = [rng.uniform(0.0, 1.0, (4000, 3)), rng.uniform(-0.25, 1.6, (1000, 3)), rng.uniform(-0.02, 0.02, (1000, 3)), grey]
        if kind == 'xyz':  # the XYZ of those RGB pixels (a random triplet is no colour: its linear RGB is far outside any range)
            with np.errstate(all='ignore'):
                parts = [A.rgb_to_xyz(p) for p in parts]
        parts.append(_branch_rgb(rng) if kind == 'rgb' else _branch_xyz(rng))
    px = np.concatenate([np.asarray(p, np.float32) for p in parts])
    assert px.shape[0] <= N_PIXELS, px.shape
    # the rest: scene-like in-gamut pixels, a colour times a brightness (uniform pixels alone are mostly bright and saturated)
    fill = (rng.uniform(0.0, 1.0, (N_PIXELS - px.shape[0], 3)) * np.maximum(rng.uniform(0.0, 1.0, (N_PIXELS - px.shape[0], 1)) ** 1.5, 0.03)).astype(np.float32)
    if kind == 'lab':
        fill[:, 1:] = (fill[:, 1:] - 0.5) * 1.2
    px = np.concatenate([px, fill])
    # no float32 denormals (outside the tested domain): flush them to zero
    px[np.abs(px) < np.finfo(np.float32).tiny] = 0.0
    px = px[rng.permutation(N_PIXELS)]
    px.setflags(write=False)
    return px


def storage(px, dtype):
    """The frame as the kernel reads it from `dtype` storage ('f32' or 'f16'), as float32."""
    if dtype == 'f32':
        return px
    with np.errstate(over='ignore'):
        h = px.astype(np.float16)
    h[np.abs(h) < np.finfo(np.float16).tiny] = 0.0   # binary16 subnormals widen to float32 normals; keep the set free of tiny values anyway
    return h.astype(np.float32)


@functools.lru_cache(maxsize=None)
def luminance_plane(log):
    """New lightness for the replace ops: inside and outside [0, 1] (the ops clamp it), on both clamps."""
    rng = np.random.default_rng(104)
    l = rng.uniform(-0.2, 1.3, N_PIXELS)
    l[::97] = 0.0
    l[1::97] = 1.0
    if log:
        l = np.log(np.maximum(l, 1e-4)) + rng.uniform(-0.2, 0.2, N_PIXELS)
    l = l.astype(np.float32)
    l.setflags(write=False)
    return l


# special values, each in every channel position (the other channels ordinary) and in all three at once
FLT_MAX = float(np.finfo(np.float32).max)
METRICS = np.array([-2.3, 0.18, 0.21, 0.19, 0.15], np.float32)
METRICS_KEY_LOW = np.array([0.5, 0.18, 0.21, 0.19, 0.15], np.float32)     # log_mean >= 0: normalized clamps to 0, map_key = 0.3
METRICS_KEY_HIGH = np.array([-12.0, 0.18, 0.21, 0.19, 0.15], np.float32)  # log_mean <= -9.21034: normalized clamps to 1, map_key = 1
SPECIALS = [0.0, -0.0, 1.0, 0.21, 0.19, 0.15, -1.0, 65504.0, FLT_MAX, np.inf, -np.inf, np.nan]


@functools.lru_cache(maxsize=None)
def special_pixels():
    px = []
    for v in SPECIALS:
        for ch in range(3):
            p = np.array([0.3, 0.6, 0.45], np.float32)
            p[ch] = v
            px.append(p)
        px.append(np.full(3, v, np.float32))
    px += [np.array(p, np.float32) for p in ((0.3, 0.6, 0.45), (0.5, 0.5, 0.5), (0.9, 0.1, 0.2))]
    px = np.array(px, np.float32)   # 51 pixels = 4 k + 3: vector body and tail
    px.setflags(write=False)
    return px


# ---------------------------------------------------------------- cases
HSL_SETS = [(0.1, 0.3, -0.2), (-0.25, -0.4, 0.5), (0.0, 0.0, 0.0)]
VIBRANCE_SETS = [(0.0,), (0.5,), (-0.3,)]
LOG_EPS = 1e-4
NORMALIZE_BOUNDS = (0.11, 0.93)   # does not contain the frame: results below 0 and above 1

# (operator key in CONSTANTS, evaluate() name, pixel kind, params)
COLOR_CASES = [(op, op, kind, None) for op, kind in [('rgb_to_xyz', 'rgb'), ('xyz_to_lab', 'xyz'), ('lab_to_xyz', 'lab'), ('xyz_to_rgb', 'xyz'),
                                                      ('rgb_to_lab', 'rgb'), ('lab_to_rgb', 'lab')]]
COLOR_CASES += [('modify_hsl', 'modify_hsl', 'rgb', p) for p in HSL_SETS]
COLOR_CASES += [('modify_vibrance', 'modify_vibrance', 'rgb', p) for p in VIBRANCE_SETS]
COLOR_CASES += [('compute_luminance', 'compute_luminance', 'rgb', None), ('compute_log_luminance', 'compute_log_luminance', 'rgb', (LOG_EPS,)),
                ('modify_luminance', 'modify_luminance', 'rgb', None), ('modify_log_luminance', 'modify_log_luminance', 'rgb', None),
                ('normalize_image', 'normalize_image', 'rgb', NORMALIZE_BOUNDS)]

INF = float('inf')
# (gamma, intensity, light_adapt, vibrance), metrics.  The first three are test_tonemaps_closed_form's; vibrance == 0 with a finite
# gamma runs the kernels' LEAN instantiation, everything else the full one
TONEMAP_SETS = [
    ((0.75, 2.0, 1.0, 0), METRICS),           # LEAN, light_adapt 1
    ((2.2, 0.5, 0.6, 0.4), METRICS),
    ((1.0, -1.0, 0.0, -0.3), METRICS),          # light_adapt 0, negative vibrance
    ((1.0, 0.0, 0.0, 0), METRICS),            # LEAN, light_adapt 0
    ((2.2, 1.0, 1.0, 0.4), METRICS),            # full, light_adapt 1
    ((INF, 0.5, 0.8, 0), METRICS),            # 1 / gamma == 0: full instantiation with vibrance 0, pow(x, 0) == 1
    ((0.75, 2.0, 0.8, 0), METRICS_KEY_LOW),   # map_key on its lower clamp
    ((0.75, 2.0, 0.8, 0.2), METRICS_KEY_HIGH),  # map_key on its upper clamp
    ((1.8, 1.0, 0.8, -0.5), METRICS),
]
TONEMAP_MODES = ['reinhard', 'aces', 'adaptive_aces', 'linear']
TONEMAP_CASES = [('tonemap_' + m, 'tonemap_' + m, 'rgb', (tuple(float(v) for v in mt),) + prm) for m in TONEMAP_MODES for prm, mt in TONEMAP_SETS]


def case_id(case):
    key, op, kind, params = case
    if params is None:
        return op
    flat = []
    for p in params:
        flat += list(p) if isinstance(p, tuple) else [p]
    if op.startswith('tonemap_'):
        flat = [flat[0]] + flat[5:]   # log_mean, gamma, intensity, light_adapt, vibrance
    return op + '-' + '_'.join(f'{v:g}' for v in flat)


def case_params(case):
    """evaluate()'s params of a case: the tone mappers take (metrics, gamma, intensity, light_adapt, vibrance)."""
    key, op, kind, params = case
    if op.startswith('tonemap_'):
        return (np.array(params[0], np.float32),) + tuple(params[1:])
    return params


def case_input(case, dtype, special=False):
    """(N, 3) or (N, 4) float32 input of a case as the kernel sees it (the luminance plane is always float32 storage)."""
    key, op, kind, params = case
    px = storage(special_pixels() if special else pixels(kind), dtype)
    if op in ('modify_luminance', 'modify_log_luminance'):
        lum = luminance_plane(op == 'modify_log_luminance')
        if special:
            lum = np.resize(np.array([0.5, 0.0, 1.0, -1.0, 2.0, np.nan, np.inf, -np.inf, 65504.0, -65504.0], np.float32), px.shape[0])
            if op == 'modify_log_luminance':
                lum = np.where(np.isfinite(lum), np.clip(lum, -20, 20), lum).astype(np.float32)
        px = np.concatenate([px, lum[:, None]], 1)
    return np.ascontiguousarray(px, np.float32)


@functools.lru_cache(maxsize=None)
def case_spec(case, dtype, special=False):
    """(input float32, result, sensitivity, scale, pre-clip result or None) of a case, computed once per session."""
    x = case_input(case, dtype, special)
    r, s, sc, pre = evaluate_with_sensitivity(case[1], x, case_params(case))
    for a in (x, r, s, sc):
        a.setflags(write=False)
    return x, r, s, sc, pre


def oracle_run(oracle, case, x):
    """The fp32 C oracle on the (N, C) input of a case: float result (N, M) (and uint8 for the tone mappers)."""
    key, op, kind, params = case
    img = np.ascontiguousarray(x[None, :, :3])
    if op.startswith('tonemap_'):
        u8, f = oracle.tonemap(op[len('tonemap_'):], img, np.array(params[0], np.float32), *params[1:], return_float=True)
        return f[0], u8[0]
    if op in ('compute_luminance', 'compute_log_luminance'):
        return oracle.compute_luminance(img, op == 'compute_log_luminance', LOG_EPS)[0][:, None], None
    if op in ('modify_luminance', 'modify_log_luminance'):
        return oracle.modify_luminance(img, np.ascontiguousarray(x[None, :, 3]), op == 'modify_log_luminance')[0], None
    if op == 'normalize_image':
        b = np.array(params, np.float32)
        with np.errstate(all='ignore'):
            return (x - b[0]) / (b[1] - b[0]), None   # reference pipeline/util.py: the float32 expression itself
    return oracle.color_op(op, img, params)[0], None


# ---------------------------------------------------------------- special pixels: what the oracle decides
def oracle_decided(oracle, case, x, u8):
    """(the oracle's output on x, mask of the values it DECIDES): a value is decided when the oracle returns the same bits
    with any one input channel moved by +-(|x| * 2^-21 + 2^-24), the specification's own perturbation, and by 32 times that (a
    finite value stays finite).  What a NaN, an overflow, a clip or a branch fixes is decided; a value that is the reference's
    own rounding noise -- the channels next to a 65504 one after the Lab round trip at 1e10, where the cancelling 3x3 product
    leaves +-1e3 -- or sits on a rounding tie is not."""
    pick = (lambda o: o[1]) if u8 else (lambda o: o[0])
    base = pick(oracle_run(oracle, case, x))
    same = np.ones(base.shape, bool)
    fmax = np.float32(FLT_MAX)
    for c in range(x.shape[1]):
        with np.errstate(all='ignore'):
            step = (np.abs(x[:, c].astype(np.float64)) * 2.0 ** -21 + 2.0 ** -24)
        for sign in (1.0, -1.0, 32.0, -32.0):
            xp = x.copy()
            with np.errstate(all='ignore'):
                moved = (x[:, c].astype(np.float64) + sign * step).astype(np.float32)
            xp[:, c] = np.where(np.isfinite(x[:, c]), np.clip(moved, -fmax, fmax), x[:, c])
            o = pick(oracle_run(oracle, case, xp))
            same &= (o == base) | (np.isnan(o) & np.isnan(base))
    return base, same


def special_classes(oracle, case):
    """Every value of a case's special frame falls in one of three classes, fixed by the oracle and the specification alone:
      exact  the oracle decides it (oracle_decided), and it is not merely an ill-conditioned value on which the oracle follows the
             float64 result: the kernel must return the oracle's value;
      tied   not exact, and the specification's GPU bound is at most 1e-3: the kernel is held to the specification as on the
             random sets (float: inside the bound; uint8: one step off only on a rounding tie);
      loose  not exact, bound above 1e-3 (ill-conditioned in the reference itself, e.g. the channels next to a 65504 one after a
             Lab round trip at 1e10): the kernel is held to the oracle's value within that bound.
    Returns (x, spec result, GPU bound, oracle output as float64, exact, tied, loose)."""
    x, r, s, sc, pre = case_spec(case, 'f32', True)
    b = bound(case[0], s, sc, pre, GPU_FACTOR)
    ex = excluded(case[0], s, sc, pre)
    u8 = case[1].startswith('tonemap_')
    o, decided = oracle_decided(oracle, case, x, u8)
    o = o.astype(np.float64)
    follows = ex & (o == (quantise(r) if u8 else r))
    exact = decided & ~follows
    return x, r, b, o, exact, ~exact & ~ex, ~exact & ex


# (exact, tied, loose) counts per case, from `python tests/color_domain_spec.py special`; tests/test_color_domain_spec.py holds the
# oracle and the specification to them, so that a change which quietly moves values out of `exact` fails
SPECIAL_COUNTS = {
    'rgb_to_xyz': (48, 93, 12),
    'xyz_to_lab': (26, 100, 27),
    'lab_to_xyz': (31, 105, 17),
    'xyz_to_rgb': (46, 89, 18),
    'rgb_to_lab': (48, 93, 12),
    'lab_to_rgb': (46, 93, 14),
    'modify_hsl-0.1_0.3_-0.2': (39, 90, 24),
    'modify_hsl--0.25_-0.4_0.5': (39, 84, 30),
    'modify_hsl-0_0_0': (63, 90, 0),
    'modify_vibrance-0': (50, 87, 16),
    'modify_vibrance-0.5': (68, 70, 15),
    'modify_vibrance--0.3': (59, 86, 8),
    'compute_luminance': (6, 45, 0),
    'compute_log_luminance-0.0001': (8, 43, 0),
    'modify_luminance': (72, 67, 14),
    'modify_log_luminance': (76, 63, 14),
    'normalize_image-0.11_0.93': (24, 111, 18),
    'tonemap_reinhard--2.3_0.75_2_1_0': (153, 0, 0),
    'tonemap_reinhard--2.3_2.2_0.5_0.6_0.4': (147, 0, 6),
    'tonemap_reinhard--2.3_1_-1_0_-0.3': (153, 0, 0),
    'tonemap_reinhard--2.3_1_0_0_0': (153, 0, 0),
    'tonemap_reinhard--2.3_2.2_1_1_0.4': (139, 0, 14),
    'tonemap_reinhard--2.3_inf_0.5_0.8_0': (153, 0, 0),
    'tonemap_reinhard-0.5_0.75_2_0.8_0': (153, 0, 0),
    'tonemap_reinhard--12_0.75_2_0.8_0.2': (153, 0, 0),
    'tonemap_reinhard--2.3_1.8_1_0.8_-0.5': (147, 0, 6),
    'tonemap_aces--2.3_0.75_2_1_0': (140, 1, 12),
    'tonemap_aces--2.3_2.2_0.5_0.6_0.4': (141, 0, 12),
    'tonemap_aces--2.3_1_-1_0_-0.3': (141, 0, 12),
    'tonemap_aces--2.3_1_0_0_0': (141, 0, 12),
    'tonemap_aces--2.3_2.2_1_1_0.4': (141, 0, 12),
    'tonemap_aces--2.3_inf_0.5_0.8_0': (129, 0, 24),
    'tonemap_aces-0.5_0.75_2_0.8_0': (140, 1, 12),
    'tonemap_aces--12_0.75_2_0.8_0.2': (140, 1, 12),
    'tonemap_aces--2.3_1.8_1_0.8_-0.5': (140, 1, 12),
    'tonemap_adaptive_aces--2.3_0.75_2_1_0': (125, 0, 28),
    'tonemap_adaptive_aces--2.3_2.2_0.5_0.6_0.4': (141, 0, 12),
    'tonemap_adaptive_aces--2.3_1_-1_0_-0.3': (141, 0, 12),
    'tonemap_adaptive_aces--2.3_1_0_0_0': (141, 0, 12),
    'tonemap_adaptive_aces--2.3_2.2_1_1_0.4': (127, 0, 26),
    'tonemap_adaptive_aces--2.3_inf_0.5_0.8_0': (129, 0, 24),
    'tonemap_adaptive_aces-0.5_0.75_2_0.8_0': (141, 0, 12),
    'tonemap_adaptive_aces--12_0.75_2_0.8_0.2': (149, 2, 2),
    'tonemap_adaptive_aces--2.3_1.8_1_0.8_-0.5': (141, 0, 12),
    'tonemap_linear--2.3_0.75_2_1_0': (138, 0, 15),
    'tonemap_linear--2.3_2.2_0.5_0.6_0.4': (136, 0, 17),
    'tonemap_linear--2.3_1_-1_0_-0.3': (145, 0, 8),
    'tonemap_linear--2.3_1_0_0_0': (136, 2, 15),
    'tonemap_linear--2.3_2.2_1_1_0.4': (130, 0, 23),
    'tonemap_linear--2.3_inf_0.5_0.8_0': (153, 0, 0),
    'tonemap_linear-0.5_0.75_2_0.8_0': (138, 0, 15),
    'tonemap_linear--12_0.75_2_0.8_0.2': (153, 0, 0),
    'tonemap_linear--2.3_1.8_1_0.8_-0.5': (140, 0, 13),
}


# ---------------------------------------------------------------- constants
# operator: (A_op, K_op, largest |oracle - spec| / bound measured over the operator's cases, largest number of uint8 values of a case, of
#            its 3 * N_PIXELS, on which the oracle differs by one step from floor(clip(spec) * 255 + 0.5))
CONSTANTS = {
    'rgb_to_xyz': (2.0 ** -30, 1, 0.495, 0),
    'xyz_to_lab': (2.0 ** -30, 1, 0.613, 0),
    'lab_to_xyz': (2.0 ** -30, 1, 0.503, 0),
    'xyz_to_rgb': (2.0 ** -30, 1, 0.582, 0),               # excluded share at most 0.0009
    'rgb_to_lab': (2.0 ** -22, 1, 0.704, 0),
    'lab_to_rgb': (2.0 ** -20, 1, 0.926, 0),               # 0.0045
    'modify_hsl': (2.0 ** -16, 32, 0.951, 0),              # 0.0047
    'modify_vibrance': (2.0 ** -17, 1, 0.705, 0),
    'compute_luminance': (2.0 ** -23, 1, 0.918, 0),
    'compute_log_luminance': (2.0 ** -22, 1, 0.933, 0),    # 0.0049
    'modify_luminance': (2.0 ** -21, 1, 0.979, 0),
    'modify_log_luminance': (2.0 ** -19, 1, 0.740, 0),
    'normalize_image': (2.0 ** -30, 1, 0.237, 0),
    'tonemap_reinhard': (2.0 ** -18, 1, 0.819, 3),    # 0.0017
    'tonemap_aces': (2.0 ** -18, 1, 0.773, 2),
    'tonemap_adaptive_aces': (2.0 ** -19, 1, 0.868, 3),  # 0.0023
    'tonemap_linear': (2.0 ** -17, 1, 0.984, 3),      # 0.0060
}


def measure_constants(oracle, verbose=True):
    """The rule of the module docstring, over every case and both storage types.  Returns {operator: (A, K, ratio, u8 share)}."""
    out = {}
    by_op = {}
    for case in COLOR_CASES + TONEMAP_CASES:
        by_op.setdefault(case[0], []).append(case)
    for key, cases in by_op.items():
        data = []
        for case in cases:
            for dtype in ('f32', 'f16'):
                x, r, s, sc, pre = case_spec(case, dtype)
                of, ou8 = oracle_run(oracle, case, x)
                data.append((case, dtype, r, s, sc, pre, _absdiff(of.astype(np.float64), r), ou8))

        def worst(a, k):
            w, share = 0.0, 0.0
            for case, dtype, r, s, sc, pre, d, ou8 in data:
                ex = excluded(key, s, sc, pre, (a, k))
                share = max(share, ex.mean())
                b = bound(key, s, sc, pre, 1.0, (a, k))
                with np.errstate(all='ignore'):
                    ratio = np.where(ex | (d == 0.0), 0.0, d / b)
                w = max(w, float(ratio.max()))
            return w, share

        passing = {}
        for ea in range(-30, int(np.log2(A_MAX)) + 1):
            for ek in range(0, 11):
                if any(pa <= ea and pk <= ek for pa, pk in passing):
                    continue   # dominated by a smaller passing pair: not minimal
                w, share = worst(2.0 ** ea, 2.0 ** ek)
                if w <= 1.0:
                    passing[(ea, ek)] = share
        (ea, ek), _ = min(passing.items(), key=lambda kv: (kv[1], kv[0][1], kv[0][0]))
        a, k = 2.0 ** ea, 2.0 ** ek
        w, share = worst(a, k)
        u8 = 0
        for case, dtype, r, s, sc, pre, d, ou8 in data:
            if ou8 is not None:
                u8 = max(u8, int((ou8.astype(np.float64) != quantise(r)).sum()))
        out[key] = (a, k, w, u8)
        if verbose:
            print(f"    '{key}': (2.0 ** {int(np.log2(a))}, {k:g}, {w:.3f}, {u8}),   # excluded share at most {share:.4f}")
    return out


if __name__ == '__main__':
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'oracle'))
    import tdk_oracle

    tdk_oracle.build()
    if sys.argv[1:] == ['special']:
        for case in COLOR_CASES + TONEMAP_CASES:
            c = special_classes(tdk_oracle, case)
            print(f"    '{case_id(case)}': ({c[4].sum()}, {c[5].sum()}, {c[6].sum()}),")
    else:
        measure_constants(tdk_oracle)
