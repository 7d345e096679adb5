"""CPU-only: the NumPy restatement tests/dehaze_spec.py of include/tdk_hip_dehaze.h, held

  * to literal loops: per-cell and per-pixel loops in float32 scalars for steps 1, 2, 4 and 5 on small frames, and a sort-based
    selection for step 3;
  * to its purpose, on a synthetic hazy scene with a fixed seed: the ambient light is recovered, the error to the haze-free scene
    falls, and the guided refinement brings the transmission closer to the truth around a depth edge than plain upsampling does.

The bounds of the purpose test are the values measured on this restatement widened by a quarter; they stand next to each assertion."""

import numpy as np
import pytest

import dehaze_spec as spec

f32 = np.float32
REC709 = spec.REC709


def frame(h, w, seed, dtype=np.float32, negative=True):
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.3, 0.9, (-(-h // 5), -(-w // 5), 3)).repeat(5, 0).repeat(5, 1)[:h, :w] + rng.normal(0, 0.08, (h, w, 3))).astype(f32)
    if negative:
        x[rng.random((h, w)) < 0.03] *= f32(-1)
    return x.astype(dtype)


# ---- literal loops
def loop_pos(v):
    return v if v > 0 else f32(0)


def loop_tree(values):
    values = list(values)
    while len(values) > 1:
        values = [values[i] + values[i + 1] for i in range(0, len(values), 2)]
    return values[0]


def loop_cells(x, s, weights):
    x = x.astype(f32)
    h, w, _ = x.shape
    ch, cw = -(-h // s), -(-w // s)
    w0, w1, w2 = (f32(v) for v in weights)
    m, mean, lum = np.zeros((ch, cw, 3), f32), np.zeros((ch, cw, 3), f32), np.zeros((ch, cw), f32)
    for cy in range(ch):
        for cx in range(cw):
            px = [[x[min(cy * s + j, h - 1), min(cx * s + i, w - 1)] for i in range(s)] for j in range(s)]
            for c in range(3):
                m[cy, cx, c] = min(loop_pos(p[c]) for row in px for p in row)
                mean[cy, cx, c] = loop_tree([loop_tree([loop_pos(p[c]) for p in row]) for row in px]) * f32(1.0 / (s * s))
            lum[cy, cx] = loop_tree([loop_tree([loop_pos((w0 * p[0] + w1 * p[1]) + w2 * p[2]) for p in row]) for row in px]) * f32(1.0 / (s * s))
    return m, mean, lum


def loop_minwin(p, r):
    h, w = p.shape
    out = np.zeros_like(p)
    for y in range(h):
        for x in range(w):
            out[y, x] = min(p[min(max(y + j, 0), h - 1), min(max(x + i, 0), w - 1)] for j in range(-r, r + 1) for i in range(-r, r + 1))
    return out


def loop_box(p, r):
    h, w = p.shape
    rows = np.zeros_like(p)
    for y in range(h):
        for x in range(w):
            acc = p[y, min(max(x - r, 0), w - 1)]
            for k in range(-r + 1, r + 1):
                acc = acc + p[y, min(max(x + k, 0), w - 1)]
            rows[y, x] = acc
    out = np.zeros_like(p)
    for y in range(h):
        for x in range(w):
            acc = rows[min(max(y - r, 0), h - 1), x]
            for k in range(-r + 1, r + 1):
                acc = acc + rows[min(max(y + k, 0), h - 1), x]
            out[y, x] = acc
    return out


def loop_taps(x, s, cells):
    q = max(2 * x + 1 - s, 0)
    return q // (2 * s), min(q // (2 * s) + 1, cells - 1), f32(q % (2 * s)) / f32(2 * s)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == f32 else np.uint16), b.view(np.uint32 if b.dtype == f32 else np.uint16))


CASES = [(13, 9, 4, 1, 2), (7, 5, 2, 2, 1), (5, 3, 8, 1, 3), (33, 18, 16, 0, 0), (20, 17, 8, 4, 8)]   # (w, h, cell, rd, rg)


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_steps_1_and_2_are_the_literal_loops(dtype):
    for k, (w, h, s, rd, _) in enumerate(CASES):
        x = frame(h, w, k, dtype)
        weights = REC709 if k % 2 == 0 else (0.25, 0.5, 0.25)
        m, mean, lum = spec.cells(x, s, weights)
        lm, lmean, llum = loop_cells(x, s, weights)
        assert same(m, lm) and same(mean, lmean) and same(lum, llum), (w, h, s)
        assert (m >= 0).all() and not np.signbit(m).any()
        low = np.minimum(np.minimum(lm[..., 0], lm[..., 1]), lm[..., 2])
        assert same(spec.dark_channel(m, rd), loop_minwin(low, rd)), (w, h, s, rd)


def test_step_3_is_a_sort_with_every_tie():
    rng = np.random.default_rng(5)
    d = rng.integers(0, 12, (9, 14)).astype(f32) / f32(16)        # many ties
    mean = rng.uniform(0, 2, (9, 14, 3)).astype(f32)
    mean[0, 0] = (70000.0, 65536.0, 65537.0)                       # the clamp of fix
    d[0, 0] = 1.0
    order = np.sort(d.ravel())[::-1]
    for count in (1, 2, 7, 60, d.size):
        threshold = order[count - 1]
        chosen = [(y, x) for y in range(9) for x in range(14) if d[y, x] >= threshold]
        assert len(chosen) >= count
        want = []
        for c in range(3):
            total = 0
            for y, x in chosen:
                total += int(min(float(mean[y, x, c]), 65536.0) * 1048576.0)   # exact in float64 too: 24 bits times a power of two
            want.append(f32((float(total) / float(len(chosen))) * 2.0 ** -20))
        want.append(f32(len(chosen)))
        got = spec.ambient(d, mean, count)
        assert same(got, np.array(want, dtype=f32)), (count, got, want)
    assert spec.ambient(d, mean, 1)[0] == f32(65536.0) and spec.ambient(d, mean, 1)[3] == 1
    assert spec.ambient(d, mean, d.size)[3] == d.size
    assert spec.count_of(0.01, 4096, 3072, 8) == 1966 and spec.count_of(0.01, 7, 5, 8) == 1 and spec.count_of(1.0, 33, 17, 4) == 9 * 5


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_steps_4_and_5_are_the_literal_loops(dtype):
    for k, (w, h, s, rd, rg) in enumerate(CASES):
        x = frame(h, w, 10 + k, dtype)
        strength, floor, eps = (f32(0.9), f32(0.1), f32(1e-3)) if k % 2 == 0 else (f32(1.0), f32(0.3), f32(1e-5))
        amb = np.array([0.8, 0.85, 0.9, 3], dtype=f32) if k != 1 else np.array([np.nan, 0.0, 0.7, 0], dtype=f32)
        m, _, lum = spec.cells(x, s)
        ch, cw = lum.shape
        big = [max(float(v), 2.0 ** -10) if v == v else 2.0 ** -10 for v in amb[:3]]
        big = [f32(v) for v in big]
        inverse = [f32(1) / v for v in big]
        q = np.zeros((ch, cw), f32)
        for cy in range(ch):
            for cx in range(cw):
                q[cy, cx] = min(min(m[cy, cx, 0] * inverse[0], m[cy, cx, 1] * inverse[1]), m[cy, cx, 2] * inverse[2])
        t = np.zeros((ch, cw), f32)
        low = loop_minwin(q, rd)
        for cy in range(ch):
            for cx in range(cw):
                t[cy, cx] = f32(1) - strength * min(low[cy, cx], f32(1))
        assert same(spec.cell_transmission(m, amb, rd, strength), t), (w, h, s, rd)
        inv = f32(1.0 / float((2 * rg + 1) ** 2))
        bl, bt, blt, bll = loop_box(lum, rg), loop_box(t, rg), loop_box(lum * t, rg), loop_box(lum * lum, rg)
        a, b = np.zeros((ch, cw), f32), np.zeros((ch, cw), f32)
        for cy in range(ch):
            for cx in range(cw):
                ml, mt = bl[cy, cx] * inv, bt[cy, cx] * inv
                cov = blt[cy, cx] * inv - ml * mt
                var = loop_pos(bll[cy, cx] * inv - ml * ml)
                a[cy, cx] = cov / (var + eps)
                b[cy, cx] = mt - a[cy, cx] * ml
        sa, sb = spec.coefficients(lum, t, rg, eps)
        assert same(sa, a) and same(sb, b), (w, h, s, rg)
        a2, b2 = loop_box(a, rg) * inv, loop_box(b, rg) * inv
        out, tp = np.zeros((h, w, 3), dtype), np.zeros((h, w), f32)
        w0, w1, w2 = (f32(v) for v in REC709)
        lerp = lambda p0, p1, f: p0 + f * (p1 - p0)
        with np.errstate(over='ignore'):
            for y in range(h):
                y0, y1, fy = loop_taps(y, s, ch)
                for xx in range(w):
                    x0, x1, fx = loop_taps(xx, s, cw)
                    p = x[y, xx].astype(f32)
                    lum_px = loop_pos((w0 * p[0] + w1 * p[1]) + w2 * p[2])
                    au = lerp(lerp(a2[y0, x0], a2[y0, x1], fx), lerp(a2[y1, x0], a2[y1, x1], fx), fy)
                    bu = lerp(lerp(b2[y0, x0], b2[y0, x1], fx), lerp(b2[y1, x0], b2[y1, x1], fx), fy)
                    tp[y, xx] = min(max(au * lum_px + bu, floor), f32(1))
                    rt = f32(1) / tp[y, xx]
                    for c in range(3):
                        out[y, xx, c] = loop_pos((p[c] - big[c]) * rt + big[c])
        got, got_tp, got_amb = spec.process(x, amb, strength, floor, s, rd, rg, eps)
        assert same(got_tp, tp) and same(got, out), (w, h, s, rd, rg)
        assert got.dtype == dtype and same(got_amb[:3][amb[:3] == amb[:3]], amb[:3][amb[:3] == amb[:3]])


def test_the_estimate_inside_process_is_estimate():
    x = frame(37, 50, 3)
    count = spec.count_of(0.05, 50, 37, 4)
    amb = spec.estimate(x, 4, 2, count)
    out, tp, used = spec.process(x, None, cell=4, dark_radius=2, radius=3, count=count)
    again, tp_again, _ = spec.process(x, amb, cell=4, dark_radius=2, radius=3)
    assert same(used, amb) and same(out, again) and same(tp, tp_again) and amb[3] >= count


def test_strength_zero_leaves_the_frame_nearly_alone():
    x = frame(40, 56, 4, negative=False)
    out, tp, _ = spec.process(x, None, strength=0.0, count=3)
    assert np.abs(tp - 1).max() < 1e-5 and np.abs(out - x).max() < 1e-5


# ---- purpose
H, W = 256, 384
NEAR = (slice(83, 197), slice(117, 259))   # the near rectangle, off the cell grid
SKY = 24


def scene(ambient_light, noise, seed=7):
    """(hazy frame, haze-free scene, true transmission): a textured scene with 5 % black pixels, t from 0.15 at the top to 0.95 at the
    bottom, a near rectangle with t = 0.9 in front of the far field, 24 rows of sky."""
    rng = np.random.default_rng(seed)
    albedo = rng.uniform(0.15, 0.8, (-(-H // 6), -(-W // 6), 3)).repeat(6, 0).repeat(6, 1)[:H, :W]
    clear = albedo * rng.uniform(0.6, 1.0, (H, W, 1))
    clear[rng.random((H, W)) < 0.05] = 0.0
    t = np.repeat(np.linspace(0.15, 0.95, H)[:, None], W, 1)
    t[NEAR] = 0.9
    light = np.asarray(ambient_light, dtype=np.float64)
    clear[:SKY] = light
    hazy = clear * t[..., None] + light * (1.0 - t[..., None])
    if noise:
        hazy = hazy + rng.normal(0.0, noise, hazy.shape)
    return hazy.astype(f32), clear.astype(f32), t.astype(f32)


def band_mask(width=8):
    yy, xx = np.mgrid[0:H, 0:W]
    y0, y1, x0, x1 = NEAR[0].start, NEAR[0].stop - 1, NEAR[1].start, NEAR[1].stop - 1
    dy = np.maximum(np.maximum(y0 - yy, yy - y1), 0)
    dx = np.maximum(np.maximum(x0 - xx, xx - x1), 0)
    outside = np.maximum(dy, dx)                                   # Chebyshev distance to the rectangle, 0 inside
    inside = np.minimum(np.minimum(yy - y0, y1 - yy), np.minimum(xx - x0, x1 - xx))
    return ((outside > 0) & (outside <= width)) | ((outside == 0) & (inside < width))


def measure(ambient_light, noise):
    hazy, clear, t = scene(ambient_light, noise)
    count = spec.count_of(0.01, W, H, 8)
    out, tp, amb = spec.process(hazy, None, count=count)
    _, plain, _ = spec.process(hazy, None, count=count, refine=False)
    band = band_mask()
    return {'ambient_error': float(np.abs(amb[:3].astype(np.float64) - np.asarray(ambient_light)).max()),
            'error_ratio': float(np.abs(out - clear).mean() / np.abs(hazy - clear).mean()),
            'band_refined': float(np.abs(tp - t)[band].mean()), 'band_plain': float(np.abs(plain - t)[band].mean()), 'cells': float(amb[3])}


@pytest.mark.parametrize('ambient_light', [(0.8, 0.85, 0.9), (0.85, 0.85, 0.85)], ids=['bluish', 'grey'])
@pytest.mark.parametrize('noise', [0.0, 0.005])
def test_purpose_on_a_hazy_scene(ambient_light, noise):
    got = measure(ambient_light, noise)
    print(ambient_light, noise, got)
    # measured on this restatement over the four cases; each bound is the worst of them widened by a quarter:
    #   ambient error    7.6e-7, 5.7e-7 without noise; 3.50e-4, 1.01e-4 with    -> 4.4e-4
    #   error ratio      0.4187, 0.4188 without noise; 0.4545, 0.4544 with      -> 0.568
    #   band, refined    0.1188, 0.1186 without noise; 0.1242, 0.1240 with      -> 0.1553
    #   refined / plain  0.681, 0.680 without noise; 0.669, 0.667 with          -> 0.851   (plain: 0.1745 .. 0.1859)
    # strength 0.9 leaves a tenth of the veil and the window of the dark channel takes the clearest cell in reach: at t = 0.24 the
    # ideal tp is 0.32, which alone leaves a third of the error
    assert got['ambient_error'] <= 4.4e-4
    assert got['error_ratio'] <= 0.568
    assert got['band_refined'] <= 0.1553
    assert got['band_refined'] <= 0.851 * got['band_plain']
    assert got['cells'] >= spec.count_of(0.01, W, H, 8)
