"""The NumPy float32 restatement of include/tdk_hip_lut.h (tdk_color_lut), shared by tests/test_colorlut_spec.py (CPU: held to an
independent float64 evaluation) and tests/test_gpu_colorlut.py (GPU: the kernel must give these bits).

Every operation of the specification is one NumPy operation on float32 arrays followed by astype(float32): one rounding per
written operation, nothing contracted.  Vectorised over the pixels; about half a second per million pixels of tetrahedral
interpolation."""

import numpy as np

F = np.float32
C255 = np.array([0x3B808081], np.uint32).view(np.float32)[0]   # the float32 nearest 1/255
TETRAHEDRAL, TRILINEAR = 'tetrahedral', 'trilinear'


def _r(x):
    return np.asarray(x).astype(F)


def load(x):
    """Storage -> float32: float32 as it is, binary16 exactly, uint8 s as (float)s * c255."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return _r(x.astype(F) * C255)
    assert x.dtype in (np.float32, np.float16), x.dtype
    return x.astype(F)


def store(v, dtype):
    """float32 -> storage: binary16 rounds to nearest even once; uint8 is rint(fmin(fmax(v, 0), 1) * 255), a NaN stores 0."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return v.astype(F)
    if dtype == np.float16:
        with np.errstate(over='ignore'):
            return v.astype(np.float16)
    assert dtype == np.uint8, dtype
    return np.rint(_r(np.fmin(_clamp0(v), F(1.0)) * F(255.0))).astype(np.uint8)


def _clamp0(t):
    """fmaxf(t, 0.0f): 0 for a NaN, +0 for -0."""
    with np.errstate(invalid='ignore'):
        return np.where(t > 0, t, F(0.0)).astype(F)


def _coordinate(x, lo, scale, entries):
    """t = fminf(fmaxf((x - lo) * scale, 0), entries - 1); k = min((int)t, entries - 2); f = t - (float)k."""
    with np.errstate(invalid='ignore', over='ignore'):
        t = _r(_r(x - F(lo)) * F(scale))
    t = np.fmin(_clamp0(t), F(entries - 1)).astype(F)
    k = np.minimum(t.astype(np.int32), entries - 2)
    return k, _r(t - k.astype(F))


def apply_matrix(rgb, m):
    m = np.asarray(m, F).reshape(9)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    with np.errstate(invalid='ignore', over='ignore'):
        rows = [_r(_r(_r(m[3 * i] * r) + _r(m[3 * i + 1] * g)) + _r(m[3 * i + 2] * b)) for i in range(3)]
    return np.stack(rows, axis=-1)


def apply_shaper(rgb, table, lo, scale):
    """table: (S,) for all channels or (3, S)."""
    table = np.asarray(table, F)
    out = np.empty_like(rgb)
    for c in range(3):
        T = table if table.ndim == 1 else table[c]
        k, f = _coordinate(rgb[..., c], lo, scale, T.shape[0])
        out[..., c] = _r(T[k] + _r(f * _r(T[k + 1] - T[k])))
    return out


def _order(fa, da, fb, db):
    """Compare-and-swap of (fraction, stride) pairs: the larger fraction first, equal ones stay."""
    s = fb > fa
    return np.where(s, fb, fa), np.where(s, db, da), np.where(s, fa, fb), np.where(s, da, db)


def apply_lut(rgb, lut, lo, scale, interpolation=TETRAHEDRAL):
    """lut: (N, N, N, 3) indexed [b, g, r]; lo, scale: three values each."""
    lut = np.asarray(lut, F)
    n = lut.shape[0]
    assert lut.shape == (n, n, n, 3)
    L = lut.reshape(-1)
    (kr, fr), (kg, fg), (kb, fb) = (_coordinate(rgb[..., c], lo[c], scale[c], n) for c in range(3))
    sr, sg, sb = 3, 3 * n, 3 * n * n
    o = ((kb * n + kg) * n + kr) * 3
    out = np.empty_like(rgb)

    def lerp(p, q, f):
        return _r(p + _r(f * _r(q - p)))

    if interpolation == TRILINEAR:
        for c in range(3):
            c00 = lerp(L[o + c], L[o + sr + c], fr)
            c10 = lerp(L[o + sg + c], L[o + sg + sr + c], fr)
            c01 = lerp(L[o + sb + c], L[o + sb + sr + c], fr)
            c11 = lerp(L[o + sg + sb + c], L[o + sg + sb + sr + c], fr)
            out[..., c] = lerp(lerp(c00, c10, fg), lerp(c01, c11, fg), fb)
        return out
    assert interpolation == TETRAHEDRAL, interpolation
    f0, d0, f1, d1, f2, d2 = fr, np.full_like(o, sr), fg, np.full_like(o, sg), fb, np.full_like(o, sb)
    f0, d0, f1, d1 = _order(f0, d0, f1, d1)     # a stable sort by descending fraction: ties stay in the order r, g, b
    f1, d1, f2, d2 = _order(f1, d1, f2, d2)
    f0, d0, f1, d1 = _order(f0, d0, f1, d1)
    o1 = o + d0
    o2 = o1 + d1
    o3 = o2 + d2
    for c in range(3):
        l0, l1, l2, l3 = L[o + c], L[o1 + c], L[o2 + c], L[o3 + c]
        out[..., c] = _r(_r(_r(l0 + _r(f0 * _r(l1 - l0))) + _r(f1 * _r(l2 - l1))) + _r(f2 * _r(l3 - l2)))
    return out


def color_lut(x, out_dtype=None, matrix=None, shaper=None, shaper_lo=0.0, shaper_scale=0.0, lut=None, lut_lo=(0.0, 0.0, 0.0),
              lut_scale=(0.0, 0.0, 0.0), interpolation=TETRAHEDRAL):
    """tdk_color_lut on an (..., 3) array of float32, float16 or uint8; lo and scale are the float32 values the call is given."""
    x = np.asarray(x)
    assert x.shape[-1] == 3
    v = load(x)
    if matrix is not None:
        v = apply_matrix(v, matrix)
    if shaper is not None:
        v = apply_shaper(v, shaper, shaper_lo, shaper_scale)
    if lut is not None:
        v = apply_lut(v, lut, lut_lo, lut_scale, interpolation)
    return store(v, x.dtype if out_dtype is None else out_dtype)


def scale_of(entries, lo, hi):
    """float32(entries - 1) / (float32(hi) - float32(lo)), every operation in float32."""
    return _r(F(entries - 1) / _r(F(hi) - F(lo)))


def of(obj, x, out_dtype=None):
    """The restatement with the tables and the very numbers of a torch_darktable.ColorLUT object."""
    return color_lut(x, out_dtype, obj.matrix, None if obj.shaper is None else obj.shaper.numpy(), obj.shaper_lo, obj.shaper_scale,
                     None if obj.lut is None else obj.lut.numpy(), obj.lut_lo, obj.lut_scale, obj.interpolation)
