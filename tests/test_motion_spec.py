"""CPU-only: the NumPy restatement of the motion block (tests/motion_spec.py) held to literal loops over cells, candidates and sites
(bit for bit) and to the block's purpose: a panned chart gives its shift on the textured tiles, no motion gives a zero field at the
default bias, four quadrants moving differently are told apart, a pan through the compensated filter reaches the variance the plain
filter reaches on a static scene, and a moving edge leaves no ghost.  No device, no library.  The figures are in DESIGN.md 3.15."""

import functools

import numpy as np
import pytest

import motion_spec as spec
import temporal_spec as tspec

F = np.float32
A_NOISE, B_NOISE = 3e-4, 2e-6
MODEL = np.array([[A_NOISE, B_NOISE, 1, 20]] * 3, F)
TEXTURE = 32     # grey levels between the darkest and the brightest value of a tile's level-0 block: "the block has texture"
PAD = 64         # the chart is larger than the frame by this much on every side, so that a crop can pan


def bits(a):
    a = np.asarray(a)
    out = a.view(np.int32 if a.dtype == np.float32 else np.int16).copy()
    out[np.isnan(a)] = -1
    return out


def noisy(rng, clean, gain=1.0):
    """Noise of the model at a gain: var = (gain a) x + (gain^2 b)."""
    return (clean + rng.normal(0.0, 1.0, clean.shape) * np.sqrt(gain * A_NOISE * clean + gain * gain * B_NOISE)).astype(F)


@functools.lru_cache(maxsize=None)
def chart(h, w, flat=False):
    """A textured chart: 64 x 96 patches of torch_darktable.synthetic (sinusoids and twelve rectangles each), so that every tile holds
    edges in both directions; the plain chart has one rectangle per few tiles and leaves most blocks with one edge direction or none.
    `flat` blanks a region of two by two tiles (in the coordinates of a crop at (0, 0)) for the texture threshold to exclude."""
    import torch
    from torch_darktable.synthetic import mosaic, synthetic_rgb

    ph, pw = 64, 96
    rows = [torch.cat([synthetic_rgb(ph, pw, 1234 + 100 * r + c, 'cpu', 0.0) for c in range(-(-w // pw))], 1) for r in range(-(-h // ph))]
    out = mosaic(torch.cat(rows, 0)[:h, :w]).numpy()[:, :, 0].astype(np.float64)
    if flat:
        out[PAD + 192 - 38:PAD + 256 + 38, PAD + 320 - 38:PAD + 448 + 38] = 0.3
    out.setflags(write=False)
    return out


def crop(big, h, w, oy=0, ox=0):
    return big[PAD + oy:PAD + oy + h, PAD + ox:PAD + ox + w]


def interior(ty, tx, h, w, shift=(0, 0), levels=spec.DEFAULT_LEVELS, box=None):
    """The tile's block at the coarsest level, and that block displaced, lie inside `box` = (top, left, bottom, right) in sites (the
    frame by default).  Outside the frame the estimator sees the clamped last row or column, which does not pan."""
    top, left, bottom, right = box or (0, 0, h, w)
    hy, hx = (spec.BLOCK_H // 2) << levels, (spec.BLOCK_W // 2) << levels
    cy, cx = spec.TILE_H * ty + spec.TILE_H // 2, spec.TILE_W * tx + spec.TILE_W // 2
    return (cy - hy + min(shift[0], 0) >= top and cy + hy + max(shift[0], 0) <= bottom and cx - hx + min(shift[1], 0) >= left and
            cx + hx + max(shift[1], 0) <= right)


def block_range(level0, ty, tx):
    b = level0[spec.BLOCK_H * ty:spec.BLOCK_H * (ty + 1), spec.BLOCK_W * tx:spec.BLOCK_W * (tx + 1)].astype(int)
    return int(b.max() - b.min())


# ------------------------------------------------------------------ 1. literal loops
def literal_pyramid(frame, scale, levels):
    x = np.asarray(frame).astype(F)
    h, w = x.shape
    fmax = lambda p, q: q if np.isnan(p) else p if np.isnan(q) else max(p, q)
    fmin = lambda p, q: q if np.isnan(p) else p if np.isnan(q) else min(p, q)
    level = np.zeros((h // 2, w // 2), np.uint8)
    with np.errstate(all='ignore'):
        for i in range(h // 2):
            for j in range(w // 2):
                q = (x[2 * i, 2 * j] + x[2 * i, 2 * j + 1]) + (x[2 * i + 1, 2 * j] + x[2 * i + 1, 2 * j + 1])
                u = fmin(fmax(q * F(scale), F(0.0)), F(1.0))
                level[i, j] = int(np.sqrt(F(u)) * F(255.0) + F(0.5))
    out = [level]
    for _ in range(levels - 1):
        ph, pw = out[-1].shape
        nxt = np.zeros(((ph + 1) // 2, (pw + 1) // 2), np.uint8)
        for r in range(nxt.shape[0]):
            for c in range(nxt.shape[1]):
                r1, c1 = min(2 * r + 1, ph - 1), min(2 * c + 1, pw - 1)
                nxt[r, c] = (int(out[-1][2 * r, 2 * c]) + int(out[-1][2 * r, c1]) + int(out[-1][r1, 2 * c]) + int(out[-1][r1, c1]) + 2) >> 2
        out.append(nxt)
    return out


def literal_cost(cur, ref, k, ty, tx, dy, dx):
    h, w = cur.shape
    cy, cx = (16 * ty + 8) >> k, (32 * tx + 16) >> k
    clamp = lambda v, n: min(max(v, 0), n - 1)
    total = 0
    for r in range(cy - 8, cy + 8):
        for c in range(cx - 16, cx + 16):
            total += abs(int(cur[clamp(r, h), clamp(c, w)]) - int(ref[clamp(r + dy, h), clamp(c + dx, w)]))
    return total


def literal_match_tile(cur, ref, ty, tx, search, zero_bias):
    levels = len(cur)
    d = None
    for k in range(levels - 1, -1, -1):
        radius, base = (search, (0, 0)) if d is None else (1, (2 * d[0], 2 * d[1]))
        best = None
        for ox in range(radius, -radius - 1, -1):        # (any order: every candidate has another key)
            for oy in range(-radius, radius + 1):
                cost = literal_cost(cur[k], ref[k], k, ty, tx, base[0] + oy, base[1] + ox)
                key = cost << 14 | (oy * oy + ox * ox) << 8 | (oy + 4) << 4 | (ox + 4)
                assert key < 1 << 32
                if best is None or key < best[0]:
                    best = (key, cost, oy, ox)
        d = (base[0] + best[2], base[1] + best[3])
    cost, zero = best[1], literal_cost(cur[0], ref[0], 0, ty, tx, 0, 0)
    if cost + zero_bias >= zero:
        d, cost = (0, 0), zero
    return (2 * d[0], 2 * d[1]), (cost, zero)


def special_frame(rng, h, w, dtype=np.float32):
    frame = (0.05 + 0.9 * rng.random((h, w))).astype(dtype)
    flat = frame.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.25, 0.0, 65504.0, 4.0, 1.0], dtype)
    at = rng.choice(flat.size, size=min(flat.size, special.size), replace=False)
    flat[at] = special[:at.size]
    return frame


@pytest.mark.parametrize('h, w, levels', [(2, 2, 4), (6, 10, 3), (34, 66, 4), (22, 14, 2), (18, 38, 1)])
def test_pyramid_agrees_with_a_loop_over_cells(h, w, levels):
    rng = np.random.default_rng(h * w)
    for dtype, white in ((np.float32, 1.0), (np.float16, 0.5)):
        frame = special_frame(rng, h, w, dtype)
        scale = spec.scale_of(white)
        got, want = spec.pyramid(frame, scale, levels), literal_pyramid(frame, scale, levels)
        assert [g.shape for g in got] == spec.level_sizes(w, h, levels) == [x.shape for x in want]
        for k in range(levels):
            assert got[k].dtype == np.uint8 and np.array_equal(got[k], want[k]), k
    assert spec.scale_of() == F(0.25) and spec.scale_of(4095.0) == F(1.0 / 16380.0)
    # the layout of a slot: every level on a multiple of 16 bytes
    at, total = spec.level_offsets(66, 34, 4)
    assert at == [0, 33 * 17 + 15, 33 * 17 + 15 + 160, 33 * 17 + 15 + 160 + 48] and total == 576 + 160 + 48 + 16 and spec.pyramid_bytes(66, 34, 4) == 2 * total
    assert spec.pyramid_bytes(2, 2, 4) == 2 * 4 * 16


@pytest.mark.parametrize('h, w, levels, search, zero_bias', [(70, 130, 3, 4, 0), (70, 130, 4, 2, 40), (34, 66, 2, 3, 0), (2, 2, 4, 4, 0), (32, 64, 1, 1, 5)])
def test_match_agrees_with_a_loop_over_tiles_and_candidates(h, w, levels, search, zero_bias):
    rng = np.random.default_rng(h + w + levels)
    base = rng.random((h + 16, w + 16))
    smooth = sum(np.roll(base, (a, b), (0, 1)) for a in range(4) for b in range(4)) / 16   # (texture with some correlation, so that a shift has a basin)
    cur, ref = smooth[8:8 + h, 8:8 + w].astype(F), (smooth[6:6 + h, 12:12 + w] + 0.01 * rng.normal(size=(h, w))).astype(F)   # ref[p + (2, -4)] ~ cur[p]
    pc, pr = spec.pyramid(cur, levels=levels), spec.pyramid(ref, levels=levels)
    field, costs = spec.match(pc, pr, w, h, search, zero_bias)
    ny, nx = spec.tiles(w, h)
    assert field.shape == (ny, nx, 2) and field.dtype == np.int16 and costs.shape == (ny, nx, 2) and costs.dtype == np.uint32
    for ty in range(ny):
        for tx in range(nx):
            d, c = literal_match_tile(pc, pr, ty, tx, search, zero_bias)
            assert tuple(field[ty, tx]) == d and tuple(costs[ty, tx]) == c, (ty, tx)
    assert (field % 2 == 0).all() and np.abs(field).max() <= spec.max_displacement(levels, search) <= spec.MAX_DISPLACEMENT
    assert (costs[..., 0] <= costs[..., 1]).all()
    zeros = spec.match(pc, pr, w, h, search, zero_bias, idx=0)
    assert not zeros[0].any() and not zeros[1].any()
    assert spec.max_displacement(4, 4) == 78 and spec.max_displacement() == 38 and spec.max_displacement(1, 1) == 2


def site_by_site(frame, state, field, model, pattern, gains, radius, thresholds, pixel_threshold, max_frames, variance_floor, out_dtype):
    """The header, one output site at a time: every site of its window is evaluated with the output tile's displacement, history sites
    and window sites outside the frame are skipped."""
    h, w = frame.shape
    t_lo, t_hi = F(thresholds[0]), F(thresholds[1])
    inv = F(1.0) / (t_hi - t_lo)
    c2 = F(np.inf) if pixel_threshold is None else F(pixel_threshold) * F(pixel_threshold)
    n_max, v_min = F(max_frames), F(variance_floor)
    first = state.idx == 0
    src, dst = (state.idx + 1) & 1, state.idx & 1
    fmax = lambda p, q: q if np.isnan(p) else p if np.isnan(q) else max(p, q)
    fmin = lambda p, q: q if np.isnan(p) else p if np.isnan(q) else min(p, q)

    @functools.lru_cache(maxsize=None)
    def terms(i, j, dy, dx):
        """(A, N, e, v, valid) of site (i, j) under the displacement (dy, dx)"""
        k = (pattern >> (2 * (2 * (i & 1) + (j & 1)))) & 3
        g = F(1.0) if gains is None else F(gains[k])
        ap, bp = g * F(model[k][0]), (g * g) * F(model[k][1])
        valid = model[k][2] != 0
        hi, hj = i + dy, j + dx
        if not first and 0 <= hi < h and 0 <= hj < w:
            A, N = F(state.acc[src][hi, hj]), F(state.cnt[src][hi, hj])
        else:
            A, N = F(0.0), F(0.0)
        if not valid:
            return A, N, F(0.0), F(0.0), False
        x = F(frame[i, j])
        var = fmax(ap * fmax(A, F(0.0)) + bp, v_min)
        return A, N, (x - A) * (x - A), var + var / fmax(N, F(1.0)), True

    out = np.zeros((h, w), out_dtype)
    acc, cnt = np.zeros((h, w), state.acc[dst].dtype), np.zeros((h, w), np.float16)
    with np.errstate(all='ignore'):
        for i in range(h):
            for j in range(w):
                dy, dx = (int(v) & ~1 for v in field[i // 32, j // 64])
                E, V = F(0.0), F(0.0)
                for ii in range(max(i - radius, 0), min(i + radius, h - 1) + 1):
                    re, rv = F(0.0), F(0.0)
                    for jj in range(max(j - radius, 0), min(j + radius, w - 1) + 1):
                        _, _, e, v, _ = terms(ii, jj, dy, dx)
                        re, rv = re + e, rv + v
                    E, V = E + re, V + rv
                A, N, e, v, valid = terms(i, j, dy, dx)
                t = E / V
                s = fmin(fmax((t_hi - t) * inv, F(0.0)), F(1.0))
                if e > c2 * v:
                    s = F(0.0)
                n1 = fmin(s * N + F(1.0), n_max) if valid else F(1.0)
                x = F(frame[i, j])
                y = x if n1 == F(1.0) else A + (x - A) / n1
                out[i, j], acc[i, j], cnt[i, j] = y, y, n1
    state.acc[dst], state.cnt[dst] = acc, cnt
    state.idx = tspec.next_index(state.idx)
    return out


@pytest.mark.parametrize('radius, state_dtype, frame_dtype', [(2, np.float32, np.float32), (3, np.float16, np.float16)], ids=['r2-float32', 'r3-float16'])
def test_compensated_filter_agrees_with_a_loop_over_sites(radius, state_dtype, frame_dtype):
    rng = np.random.default_rng(17 + radius)
    h, w = 34, 66   # two by two tiles, the second row and column two sites wide
    model = np.array([[3e-4, 2e-6, 1, 9], [2e-4, 1e-6, 0 if radius == 3 else 1, 9], [5e-4, 0.0, 1, 9]], F)
    gains = None if radius == 2 else np.array([2.0, 1.0, 1.5], F)
    kw = dict(gains=gains, radius=radius, thresholds=(1.5, 3.0), pixel_threshold=4.0, max_frames=8.0, variance_floor=1e-12)
    clean = 0.1 + 0.6 * np.linspace(0, 1, w)[None, :] * np.ones((h, 1))
    fields = [np.zeros((2, 2, 2), np.int16), np.array([[[2, -4], [0, 2]], [[-2, 0], [4, 6]]], np.int16),
              np.array([[[-30, 0], [3, -5]], [[0, 70], [32767, -32768]]], np.int16), np.array([[[40, 2], [-2, 0]], [[-7, 9], [2, 0]]], np.int16)]
    sa, sb = tspec.State((h, w), state_dtype), tspec.State((h, w), state_dtype, fill=0.25)
    for f, field in enumerate(fields):
        frame = (clean + rng.normal(0, 1, (h, w)) * np.sqrt(3e-4 * clean + 2e-6)).astype(frame_dtype)
        if f == 2:
            frame[1, 2], frame[5, 7], frame[33, 65], frame[0, 0] = np.nan, np.inf, -np.inf, -0.25
        a = spec.compensated_step(frame, sa, field, model, tspec.GRBG, out_dtype=frame_dtype, **kw)
        b = site_by_site(frame, sb, field, model, tspec.GRBG, out_dtype=frame_dtype, **kw)
        assert a.dtype == b.dtype == frame_dtype and np.array_equal(bits(a), bits(b)), f
        assert sa.idx == sb.idx == f + 1
        p = f & 1
        assert np.array_equal(bits(sa.acc[p]), bits(sb.acc[p])) and np.array_equal(bits(sa.cnt[p]), bits(sb.cnt[p])), f
    assert (sa.cnt[1] > 1).any() and (sa.cnt[1] == 1).any()


def test_a_zero_field_is_the_plain_filter_and_states_change_hands():
    rng = np.random.default_rng(3)
    h, w = 40, 70
    clean = 0.1 + 0.6 * np.linspace(0, 1, w)[None, :] * np.ones((h, 1))
    zero = np.zeros((2, 2, 2), np.int16)
    odd = np.array([[[1, 1], [1, -1]], [[-1, 1], [1, 1]]], np.int16)   # -1 & ~1 = -2: a real displacement; 1 & ~1 = 0
    sa, sb = tspec.State((h, w)), tspec.State((h, w))
    for f in range(5):
        frame = noisy(rng, clean)
        field = zero if f != 3 else np.array([[[1, 1], [1, 1]], [[1, 1], [1, 1]]], np.int16)
        a = spec.compensated_step(frame, sa, field, MODEL, tspec.RGGB) if f % 2 else tspec.step(frame, sa, MODEL, tspec.RGGB)   # the state goes back and forth
        b = tspec.step(frame, sb, MODEL, tspec.RGGB)
        assert np.array_equal(bits(a), bits(b)) and sa.idx == sb.idx
        for p in (0, 1):
            assert np.array_equal(bits(sa.acc[p]), bits(sb.acc[p])) and np.array_equal(bits(sa.cnt[p]), bits(sb.cnt[p]))
    moved = spec.compensated_step(noisy(rng, clean), sa, odd, MODEL, tspec.RGGB)
    assert not np.array_equal(bits(moved), bits(tspec.step(noisy(rng, clean), sb, MODEL, tspec.RGGB)))


# ------------------------------------------------------------------ 2. purpose: the estimator
H, W = 512, 768


def pan_result(shift, gain, seed=1):
    """(tiles that were asked, tiles that were wrong) for a pan of the chart by `shift`: ref[p + shift] = cur[p]."""
    big = chart(H + 2 * PAD, W + 2 * PAD, flat=True)
    cur, ref = crop(big, H, W), crop(big, H, W, -shift[0], -shift[1])
    level0 = spec.grey(cur.astype(F), spec.scale_of())
    if gain:
        rng = np.random.default_rng(seed)
        cur, ref = noisy(rng, cur, gain), noisy(rng, ref, gain)
    field, costs = spec.estimate(cur.astype(F), ref.astype(F), zero_bias=spec.DEFAULT_ZERO_BIAS)
    ny, nx = spec.tiles(W, H)
    asked = [(ty, tx) for ty in range(ny) for tx in range(nx) if interior(ty, tx, H, W, shift) and block_range(level0, ty, tx) >= TEXTURE]
    flat = [(ty, tx) for ty in range(ny) for tx in range(nx) if block_range(level0, ty, tx) < TEXTURE]
    wrong = [t for t in asked if tuple(field[t]) != shift]
    return asked, wrong, flat, field


SHIFTS = [(0, -2), (2, 2), (4, -4), (6, -10), (-14, 22), (38, -38), (-20, -36)]


@pytest.mark.parametrize('shift', SHIFTS)
def test_a_panned_chart_gives_its_shift_on_the_textured_tiles(shift):
    """A 768 x 512 crop of the chart panned by an even shift up to max_displacement = 38.  Asked are the tiles whose level-0 block spans
    at least TEXTURE = 32 grey levels (eight flat tiles span 0, the others 65 and more) and whose coarsest block, displaced, lies inside
    the frame.  Without noise every one of them gives the shift; with model noise at gain 1 and gain 4 (a 3e-4 / b 2e-6, and 1.2e-3 /
    3.2e-5) at most 2 % may miss.  Measured: none misses, for every shift of the list."""
    assert max(abs(v) for v in shift) <= spec.max_displacement()
    asked, wrong, flat, field = pan_result(shift, 0)
    print(f'shift {shift} noiseless: {len(wrong)} of {len(asked)} textured tiles wrong, {len(flat)} flat tiles')
    assert len(asked) >= 60 and not wrong
    core = [(6, 5), (6, 6), (7, 5), (7, 6)]   # flat in both frames, whatever the shift: nothing to match, the zero preference holds them
    assert set(core) <= set(flat) and all(tuple(field[t]) == (0, 0) for t in core)
    for gain in (1.0, 4.0):
        asked, wrong, _, _ = pan_result(shift, gain)
        print(f'shift {shift} gain {gain}: {len(wrong)} of {len(asked)} textured tiles wrong')
        assert len(wrong) <= 0.02 * len(asked)


def test_a_half_sample_shift_at_level_one_is_a_known_weakness():
    """A shift of (2, 0) sites is half a sample of level 1 in one axis and nothing in the other: the candidates (0, 0) and (1, 0) of
    level 1 both miss by half a sample, on some tiles a diagonal neighbour wins by a few per cent, and the +-1 refinement of level 0
    cannot come back.  Measured without noise: 14 of 88 textured tiles are off, each by 2 sites in one axis.  Recorded, and held to
    what it is: an error of at most 2 sites per axis, on at most a quarter of the tiles."""
    asked, wrong, _, field = pan_result((2, 0), 0)
    print(f'shift (2, 0): {len(wrong)} of {len(asked)} textured tiles wrong: {sorted(set(tuple(int(v) for v in field[t]) for t in wrong))}')
    assert len(wrong) <= 0.25 * len(asked)
    assert all(abs(int(field[t][0]) - 2) <= 2 and abs(int(field[t][1])) <= 2 for t in asked)


def test_no_motion_gives_a_zero_field_at_the_default_bias():
    """The chart of torch_darktable.synthetic with fresh model noise on both frames and no motion, at gain 1 and gain 4, six pairs each:
    every tile is zero.  The default, 300, is twice the smallest bias (150, at gain 4; 79 at gain 1) at which every tile of 20 pairs
    came out zero; here the smallest sufficient bias of every pair is printed and must stay below the default."""
    from torch_darktable.synthetic import synthetic_bayer

    assert spec.DEFAULT_ZERO_BIAS == 300
    h, w = 384, 512
    clean = synthetic_bayer(h, w, seed=1234, device='cpu', noise_sigma=0.0).numpy()[:, :, 0].astype(np.float64)
    for gain in (1.0, 4.0):
        rng = np.random.default_rng(int(gain))
        need = []
        for _ in range(6):
            a, b = noisy(rng, clean, gain), noisy(rng, clean, gain)
            field, costs = spec.estimate(a, b, zero_bias=0)
            need.append(int((costs[..., 1].astype(np.int64) - costs[..., 0]).max()))
            assert need[-1] < spec.DEFAULT_ZERO_BIAS
        field, _ = spec.estimate(a, b, zero_bias=spec.DEFAULT_ZERO_BIAS)
        assert not field.any()
        sigma_grey = float((spec.grey(a, spec.scale_of()).astype(float) - spec.grey(clean.astype(F), spec.scale_of())).std())
        print(f'gain {gain}: smallest sufficient bias per pair {need}; noise {sigma_grey:.2f} grey levels, 23 sigma = {23 * sigma_grey:.0f}')


def test_four_quadrants_moving_differently_are_told_apart():
    """Each quadrant of the reference frame is the chart panned by its own shift.  Asked are the textured tiles whose coarsest block,
    displaced, lies inside their quadrant: every one gives the shift of its quadrant, with and without noise."""
    big = chart(H + 2 * PAD, W + 2 * PAD)
    shifts = {(0, 0): (6, -10), (0, 1): (-4, 8), (1, 0): (0, -6), (1, 1): (-8, -2)}
    cur = crop(big, H, W)
    ref = np.empty_like(cur)
    for (qy, qx), s in shifts.items():
        sl = (slice(qy * H // 2, (qy + 1) * H // 2), slice(qx * W // 2, (qx + 1) * W // 2))
        ref[sl] = crop(big, H, W, -s[0], -s[1])[sl]
    level0 = spec.grey(cur.astype(F), spec.scale_of())
    for gain in (0, 1.0):
        rng = np.random.default_rng(4)
        a, b = (cur.astype(F), ref.astype(F)) if not gain else (noisy(rng, cur, gain), noisy(rng, ref, gain))
        field, _ = spec.estimate(a, b, zero_bias=spec.DEFAULT_ZERO_BIAS)
        asked = 0
        for (qy, qx), s in shifts.items():
            box = (qy * H // 2, qx * W // 2, (qy + 1) * H // 2, (qx + 1) * W // 2)
            for ty in range(H // 32):
                for tx in range(W // 64):
                    if interior(ty, tx, H, W, s, box=box) and block_range(level0, ty, tx) >= TEXTURE:
                        asked += 1
                        assert tuple(field[ty, tx]) == s, (gain, ty, tx, tuple(field[ty, tx]), s)
        assert asked >= 16


# ------------------------------------------------------------------ 3. purpose: the compensated filter
@functools.lru_cache(maxsize=None)
def pan_figures(step, radius, frames=8, h=384, w=640):
    """Eight noisy frames of the chart panned by `step` sites per frame through MotionTemporalDenoise (the restatement's Sequence) and
    through the plain filter.  On the tiles whose coarsest block and whose whole history stayed inside the frame: the mean of
    (out - clean)^2 / (a clean + b) of the last frame, times 8 for the compensated filter (an ideal mean of 8 frames gives 1), and as it
    is for the plain one (the frame itself gives 1)."""
    big = chart(h + 2 * PAD, w + 2 * PAD)
    rng = np.random.default_rng(7)
    seq, plain = spec.Sequence((h, w), zero_bias=spec.DEFAULT_ZERO_BIAS), tspec.State((h, w))
    mask = np.zeros((h, w), bool)
    reach = ((frames - 1) * abs(step[0]), (frames - 1) * abs(step[1]))
    for ty in range(h // 32):
        for tx in range(w // 64):
            if interior(ty, tx, h, w, reach) and interior(ty, tx, h, w, (-reach[0], -reach[1])):
                mask[32 * ty:32 * ty + 32, 64 * tx:64 * tx + 64] = True
    for f in range(frames):
        clean = crop(big, h, w, f * step[0], f * step[1])
        x = noisy(rng, clean)
        out = seq.step(x, MODEL, tspec.RGGB, radius=radius, max_frames=float(frames))
        out_plain = tspec.step(x, plain, MODEL, tspec.RGGB, radius=radius, max_frames=float(frames))
        if f:
            right = [tuple(seq.field[ty, tx]) == step for ty in range(h // 32) for tx in range(w // 64) if mask[32 * ty, 64 * tx]]
            assert all(right), (f, step)
    var = A_NOISE * clean + B_NOISE
    assert mask.sum() >= 30 * 2048
    return float(np.mean(((out - clean) ** 2 / var)[mask])) * frames, float(np.mean(((out_plain - clean) ** 2 / var)[mask]))


@pytest.mark.parametrize('step, radius', [((0, -2), 2), ((2, 2), 3), ((4, -4), 2), ((-4, 0), 3)])
def test_a_pan_through_the_compensated_filter_reaches_the_static_figure(step, radius):
    """A pan of 2 and of 4 sites per frame, eight frames, max_frames = 8.  Measured: the static scene gives 1.010 (radius 2) and 1.004
    (radius 3) of the ideal mean of eight frames; the pans give 1.007-1.017 at radius 2 and 1.001-1.013 at radius 3.  Held: 1.10, the
    cap tests/test_temporal_spec.py holds the static scene to (its figures were 1.003-1.084).  On the same pan the plain filter leaves
    0.94-0.99 of the frame's own variance: it restarts everywhere."""
    static, _ = pan_figures((0, 0), radius)
    figure, plain = pan_figures(step, radius)
    print(f'step {step} radius {radius}: compensated {figure:.4f} of the ideal mean of 8 (static {static:.4f}); plain filter {plain:.4f} of the frame variance')
    assert static <= 1.10 and figure <= 1.10
    assert plain > 0.5 and figure / 8 < 0.25   # the need: without compensation the pan leaves more than half of the noise, with it an eighth


@pytest.mark.parametrize('radius', [2, 3])
@pytest.mark.parametrize('sigmas', [5, 10])
def test_moving_edge_leaves_no_ghost_with_compensation_on(radius, sigmas):
    """The scene of tests/test_temporal_spec.py: a vertical edge of `sigmas` noise sigmas moves 3 columns per frame over a flat 0.2
    field, through the estimator and the compensated filter.  In the 12 columns swept last, from the tenth frame on,
    |mean(out - clean)| <= 0.1 sigma and the rms <= 1.05 sigma, the bounds of the plain filter's test.  Measured: bias 0.003-0.030,
    rms 0.87-0.92; at 10 sigma the tiles on the edge follow it (37 non-zero displacements in 16 frames), at 5 sigma none moves."""
    rng = np.random.default_rng(10 * radius + sigmas)
    h, w = 96, 128
    sigma = np.sqrt(A_NOISE * 0.2 + B_NOISE)
    seq = spec.Sequence((h, w), zero_bias=spec.DEFAULT_ZERO_BIAS)
    errors, moved = [], 0
    for f in range(16):
        edge = 20 + 3 * f
        clean = np.full((h, w), 0.2)
        clean[:, :edge] += sigmas * sigma
        out = seq.step(noisy(rng, clean), MODEL, tspec.RGGB, radius=radius)
        moved += int((seq.field != 0).any(-1).sum())
        if f >= 10:
            errors.append(((out.astype(np.float64) - clean) / sigma)[:, edge - 12:edge])
    errors = np.concatenate(errors)
    bias, rms = abs(float(errors.mean())), float(np.sqrt((errors ** 2).mean()))
    print(f'radius {radius}, edge of {sigmas} sigma: bias {bias:.4f} sigma, rms {rms:.4f} sigma, {moved} displaced tiles')
    assert bias <= 0.1 and rms <= 1.05
