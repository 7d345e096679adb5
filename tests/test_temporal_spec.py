"""CPU-only: the NumPy restatement of the temporal denoiser (tests/temporal_spec.py) held to a second, per-site evaluation of the
header's formulas (bit for bit) and to the algorithm's purpose: on a static scene the filter approaches the variance of an ideal
recursive mean, a moving edge leaves no ghost, a non-finite sample is gone from the state one frame later.  No device, no library."""

import numpy as np
import pytest

import temporal_spec as spec

F = np.float32
A_NOISE, B_NOISE = 3e-4, 2e-6
MODEL = np.array([[A_NOISE, B_NOISE, 1, 20]] * 3, F)


def bits(a):
    """The bit patterns, with every NaN as one pattern: which NaN an operation returns is not part of the specification."""
    a = np.asarray(a)
    out = a.view(np.int32 if a.dtype == np.float32 else np.int16).copy()
    out[np.isnan(a)] = -1
    return out


# ------------------------------------------------------------------ 1. a second evaluation
def site_by_site(frame, state, model, pattern, gains, radius, thresholds, pixel_threshold, max_frames, variance_floor, out_dtype):
    """The header, one site at a time with NumPy float32 scalars; the window skips the sites outside the frame instead of adding zeros."""
    h, w = frame.shape
    t_lo, t_hi = F(thresholds[0]), F(thresholds[1])
    inv = F(1.0) / (t_hi - t_lo)
    c2 = F(np.inf) if pixel_threshold is None else F(pixel_threshold) * F(pixel_threshold)
    n_max, v_min = F(max_frames), F(variance_floor)
    first = state.idx == 0
    src, dst = (state.idx + 1) & 1, state.idx & 1
    fmax = lambda p, q: q if np.isnan(p) else p if np.isnan(q) else max(p, q)
    fmin = lambda p, q: q if np.isnan(p) else p if np.isnan(q) else min(p, q)
    e, v = np.zeros((h, w), F), np.zeros((h, w), F)
    A, N, valid = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), bool)
    with np.errstate(all='ignore'):
        for i in range(h):
            for j in range(w):
                k = (pattern >> (2 * (2 * (i & 1) + (j & 1)))) & 3
                g = F(1.0) if gains is None else F(gains[k])
                ap, bp = g * F(model[k][0]), (g * g) * F(model[k][1])
                valid[i, j] = model[k][2] != 0
                A[i, j] = F(0.0) if first else F(state.acc[src][i, j])
                N[i, j] = F(0.0) if first else F(state.cnt[src][i, j])
                if valid[i, j]:
                    x = F(frame[i, j])
                    var = fmax(ap * fmax(A[i, j], F(0.0)) + bp, v_min)
                    v[i, j] = var + var / fmax(N[i, j], F(1.0))
                    e[i, j] = (x - A[i, j]) * (x - A[i, j])
        out = np.zeros((h, w), out_dtype)
        acc, cnt = np.zeros((h, w), state.acc[dst].dtype), np.zeros((h, w), np.float16)
        for i in range(h):
            for j in range(w):
                E, V = F(0.0), F(0.0)
                for ii in range(max(i - radius, 0), min(i + radius, h - 1) + 1):
                    re, rv = F(0.0), F(0.0)
                    for jj in range(max(j - radius, 0), min(j + radius, w - 1) + 1):
                        re, rv = re + e[ii, jj], rv + v[ii, jj]
                    E, V = E + re, V + rv
                t = E / V
                s = fmin(fmax((t_hi - t) * inv, F(0.0)), F(1.0))
                if e[i, j] > c2 * v[i, j]:
                    s = F(0.0)
                n1 = fmin(s * N[i, j] + F(1.0), n_max) if valid[i, j] else F(1.0)
                x = F(frame[i, j])
                y = x if n1 == F(1.0) else A[i, j] + (x - A[i, j]) / n1
                out[i, j], acc[i, j], cnt[i, j] = y, y, n1
    state.acc[dst], state.cnt[dst] = acc, cnt
    state.idx = spec.next_index(state.idx)
    return out


@pytest.mark.parametrize('radius', [2, 3])
@pytest.mark.parametrize('state_dtype, frame_dtype', [(np.float32, np.float32), (np.float16, np.float16)], ids=['float32', 'float16'])
def test_vectorised_and_per_site_evaluations_agree_bit_for_bit(radius, state_dtype, frame_dtype):
    rng = np.random.default_rng(17)
    h, w = 10, 12
    model = np.array([[3e-4, 2e-6, 1, 9], [2e-4, 1e-6, 0 if radius == 3 else 1, 9], [5e-4, 0.0, 1, 9]], F)
    gains = None if radius == 2 else np.array([2.0, 1.0, 1.5], F)
    kw = dict(gains=gains, radius=radius, thresholds=(1.5, 3.0), pixel_threshold=4.0, max_frames=8.0, variance_floor=1e-12)
    clean = 0.1 + 0.6 * np.linspace(0, 1, w)[None, :] * np.ones((h, 1))
    sa, sb = spec.State((h, w), state_dtype), spec.State((h, w), state_dtype, fill=0.25)
    for f in range(4):
        frame = (clean + rng.normal(0, 1, (h, w)) * np.sqrt(3e-4 * clean + 2e-6)).astype(frame_dtype)
        if f == 2:
            frame[1, 2], frame[5, 7], frame[9, 11], frame[0, 0], frame[4, 4], frame[6, 1], frame[3, 10] = np.nan, np.inf, -np.inf, -0.25, 0.0, 65504.0, -0.0
            frame[6:9, 3:6] += 0.3   # motion
        a = spec.step(frame, sa, model, spec.GRBG, out_dtype=frame_dtype, **kw)
        b = site_by_site(frame, sb, model, spec.GRBG, out_dtype=frame_dtype, **kw)
        assert a.dtype == b.dtype == frame_dtype
        assert np.array_equal(bits(a), bits(b)), f
        assert sa.idx == sb.idx == f + 1
        p = f & 1
        assert np.array_equal(bits(sa.acc[p]), bits(sb.acc[p])) and np.array_equal(bits(sa.cnt[p]), bits(sb.cnt[p])), f
    assert (sa.cnt[1] > 1).any() and (sa.cnt[1] == 1).any()   # both branches of the update were taken


def test_the_index_advances_and_wraps():
    assert [spec.next_index(i) for i in (0, 1, 2, 0xFFFFFFFE, 0xFFFFFFFF)] == [1, 2, 3, 0xFFFFFFFF, 2]
    # the wrap keeps the parity going: 0xFFFFFFFF writes the planes 1, index 2 writes the planes 0
    assert (0xFFFFFFFF & 1, spec.next_index(0xFFFFFFFF) & 1) == (1, 0)
    assert spec.state_bytes(6, 4) == 16 + 2 * 96 + 2 * 48 and spec.state_bytes(6, 4, np.float16) == 16 + 4 * 48
    assert spec.state_bytes(2, 2) == 16 + 2 * 16 + 2 * 16   # 8 bytes of counts take a plane of 16


# ------------------------------------------------------------------ 2. quality
def noisy(rng, clean):
    return (clean + rng.normal(0.0, 1.0, clean.shape) * np.sqrt(A_NOISE * clean + B_NOISE)).astype(F)


@pytest.mark.parametrize('radius', [2, 3])
@pytest.mark.parametrize('n_max, cap', [(4, 1.10), (8, 1.10), (16, 1.15)])
def test_static_scene_reaches_the_ideal_recursive_mean(radius, n_max, cap):
    """A 96 x 128 ramp from 0.05 to 0.85, 4 n_max + 16 frames: the mean of (out - clean)^2 / (a clean + b) over the last 16 frames times
    2 n_max - 1 (the steady state of an ideal recursive mean with weight 1 / n_max is 1 / (2 n_max - 1)) is at most `cap`.  A float32
    prototype of the formulas with three seeds gave 1.003-1.024 at n_max = 4 and 8, 1.036-1.082 at 16; radius 1 fails."""
    rng = np.random.default_rng(100 * radius + n_max)
    clean = np.broadcast_to(np.linspace(0.05, 0.85, 128), (96, 128)).astype(np.float64)
    state = spec.State(clean.shape)
    frames = 4 * n_max + 16
    ratios = []
    for f in range(frames):
        out = spec.step(noisy(rng, clean), state, MODEL, spec.RGGB, radius=radius, max_frames=float(n_max))
        if f >= frames - 16:
            ratios.append(np.mean((out.astype(np.float64) - clean) ** 2 / (A_NOISE * clean + B_NOISE)))
    figure = float(np.mean(ratios)) * (2 * n_max - 1)
    print(f'radius {radius} n_max {n_max}: {figure:.4f} (cap {cap})')
    assert figure <= cap


@pytest.mark.parametrize('radius', [2, 3])
@pytest.mark.parametrize('sigmas', [5, 10])
def test_moving_edge_leaves_no_ghost(radius, sigmas):
    """A vertical edge of `sigmas` noise sigmas moves 3 columns per frame over a flat 0.2 field.  In the 12 columns swept last, from the
    tenth frame on, |mean(out - clean)| <= 0.1 sigma and the rms <= 1.05 sigma: no worse than the frame itself.  (The prototype gave
    at most 0.012, and 0.86 / 0.94.)"""
    rng = np.random.default_rng(10 * radius + sigmas)
    h, w = 96, 128
    sigma = np.sqrt(A_NOISE * 0.2 + B_NOISE)
    state = spec.State((h, w))
    errors = []
    for f in range(16):
        edge = 20 + 3 * f   # columns left of `edge` are raised
        clean = np.full((h, w), 0.2)
        clean[:, :edge] += sigmas * sigma
        out = spec.step(noisy(rng, clean), state, MODEL, spec.RGGB, radius=radius)
        if f >= 10:
            errors.append(((out.astype(np.float64) - clean) / sigma)[:, edge - 12:edge])
    errors = np.concatenate(errors)
    bias, rms = abs(float(errors.mean())), float(np.sqrt((errors ** 2).mean()))
    print(f'radius {radius}, edge of {sigmas} sigma: bias {bias:.4f} sigma, rms {rms:.4f} sigma')
    assert bias <= 0.1 and rms <= 1.05


@pytest.mark.parametrize('radius', [2, 3])
def test_non_finite_samples_are_gone_one_frame_later(radius):
    rng = np.random.default_rng(5)
    clean = np.broadcast_to(np.linspace(0.05, 0.85, 40), (24, 40)).astype(np.float64)
    state = spec.State(clean.shape)
    where = [(3, 4), (12, 20), (23, 39)]
    for f in range(1, 6):
        frame = noisy(rng, clean)
        if f == 3:
            for at, value in zip(where, (np.nan, np.inf, -np.inf)):
                frame[at] = value
        out = spec.step(frame, state, MODEL, spec.RGGB, radius=radius)
        acc, cnt = state.next_read()
        bad = np.zeros(clean.shape, bool)
        if f == 3:
            for at in where:
                bad[at] = True
            # the sites whose window holds one of them restart from the frame
            for i, j in where:
                window = cnt[max(i - radius, 0):i + radius + 1, max(j - radius, 0):j + radius + 1]
                assert (window == 1).all()
        assert np.array_equal(~np.isfinite(acc), bad) and np.array_equal(~np.isfinite(out), bad), f
        assert np.isfinite(cnt).all() and (cnt >= 1).all() and (cnt <= 8).all(), f
        if f == 4:
            for i, j in where:   # ... and once more, since the average they would continue is not finite
                assert (cnt[max(i - radius, 0):i + radius + 1, max(j - radius, 0):j + radius + 1] == 1).all()
    assert (cnt > 1).mean() > 0.9


# ------------------------------------------------------------------ 3. identities
def test_identities():
    rng = np.random.default_rng(6)
    clean = np.broadcast_to(np.linspace(0.05, 0.85, 30), (20, 30)).astype(np.float64)
    frames = [noisy(rng, clean) for _ in range(4)]
    # first: the frame passes through, whatever the planes hold
    for fill in (np.nan, 0.0, 7.0):
        state = spec.State(clean.shape, fill=fill)
        out = spec.step(frames[0], state, MODEL, spec.RGGB)
        assert np.array_equal(bits(out), bits(frames[0])) and (state.cnt[0] == 1).all() and np.array_equal(bits(state.acc[0]), bits(frames[0]))
    # ... and again after a reset
    state.reset()
    assert np.array_equal(bits(spec.step(frames[1], state, MODEL, spec.RGGB)), bits(frames[1])) and state.idx == 1
    # n_max = 1: the input's bits, always
    state = spec.State(clean.shape)
    for frame in frames:
        assert np.array_equal(bits(spec.step(frame, state, MODEL, spec.RGGB, max_frames=1.0)), bits(frame))
        assert (state.next_read()[1] == 1).all()
    # an all-zero model knows no noise: every difference is motion
    state = spec.State(clean.shape)
    zero = np.array([[0.0, 0.0, 1, 0]] * 3, F)
    for frame in frames:
        assert np.array_equal(spec.step(frame, state, zero, spec.RGGB), frame)
    # an invalid row: its sites pass through with a count of 1, the others are filtered
    state = spec.State(clean.shape)
    model = MODEL.copy()
    model[1, 2] = 0
    green = spec.rows_of(clean.shape, spec.RGGB) == 1
    for frame in frames:
        out = spec.step(frame, state, model, spec.RGGB)
        assert np.array_equal(bits(out[green]), bits(frame[green])) and (state.next_read()[1][green] == 1).all()
    assert (out[~green] != frames[-1][~green]).mean() > 0.9 and (state.next_read()[1][~green] > 1).mean() > 0.9
    # the output type rounds the same value once; the state keeps its own type
    s32, s16 = spec.State(clean.shape), spec.State(clean.shape)
    for frame in frames:
        a, b = spec.step(frame, s32, MODEL, spec.RGGB), spec.step(frame, s16, MODEL, spec.RGGB, out_dtype=np.float16)
        assert b.dtype == np.float16 and np.array_equal(bits(a.astype(np.float16)), bits(b))
