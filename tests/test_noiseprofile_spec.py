"""CPU-only: the NumPy restatement of the noise profile (tests/noiseprofile_spec.py, the yardstick of tests/test_gpu_noiseprofile.py)
held to independent evaluations -- a per-block loop in plain Python, the level edges, numpy.polyfit, float64 formulas of the
transform -- and to the accuracy chart of the issue.

Accuracy chart (512 x 768 RGGB, 8 x 8 flat patches at geomspace(0.01, 0.9, 64), CFA factors (0.6, 1, 1, 0.8), Gaussian noise of
variance a*x + b rounded to 16 bits, default_rng(0..2), min_count = 16).  The float64 prototype of these formulas had a worst error
of a of 3.1 % over the 27 fits and a mean standard deviation of the stabilised green plane within 1.1 % of sigma_out; the test holds
the restatement to 6 % and 3 %, twice the measured worst, because three seeds do not bound the tail.  b is not held there: where a*x
dominates the darkest patch the intercept is an extrapolation and comes out low (the prototype: 0.58 .. 0.98 of the truth in the
shot-noise cases, within 2 % in the read-noise case).  With (a, b) = (0, 1e-4) the fit must give |a| < 1e-5 and b within 3 %."""

import math

import numpy as np
import pytest

import noiseprofile_spec as spec

F = np.float32
CASES = [(2e-4, 1e-6), (5e-5, 4e-6), (1e-3, 1e-5)]
CFA = (0.6, 1.0, 1.0, 0.8)


# ------------------------------------------------------------------ levels
def test_level_edges_are_monotone_and_invert_the_level_function():
    edges = [spec.level_edge(l) for l in range(1, spec.LEVELS + 1)]
    assert edges[0] == 256 and all(b > a for a, b in zip(edges, edges[1:]))
    assert spec.level(0) == 0 and spec.level(255) == 0 and spec.level(256) == 1
    for l in range(2, spec.LEVELS):
        assert spec.level(spec.level_edge(l)) == l, l
        assert spec.level(spec.level_edge(l) - 1) == l - 1, l
    assert spec.level(spec.level_edge(1)) == 1 and spec.level(spec.level_edge(1) - 1) == 0
    # four levels per octave: the edges of an octave are 4, 5, 6, 7 times a power of two
    assert [spec.level_edge(l) for l in (1, 2, 3, 4, 5)] == [256, 320, 384, 448, 512]
    # the largest energy a block can have (96 second differences of 2 * 65535) lands in the last level, which the median never uses
    assert spec.level(96 * (2 * 65535) ** 2) == spec.LEVELS - 1 and spec.level(1 << 62) == spec.LEVELS - 1
    # against the definition by floor(log2) on exact integers
    rng = np.random.default_rng(5)
    for e in [int(v) for v in rng.integers(256, 1 << 41, size=2000)] + [2 ** k + d for k in range(8, 41) for d in (-1, 0, 1)]:
        want = max(l for l in range(0, spec.LEVELS) if l == 0 or spec.level_edge(l) <= e)
        assert spec.level(e) == want, e


# ------------------------------------------------------------------ block statistics, by a loop over sites
def brute_force(frames, pattern, bins, white, clip):
    hist = np.zeros((3, bins, spec.LEVELS), np.int64)
    sums, counters = np.zeros((3, bins), np.int64), np.zeros((3, 3), np.int64)
    scale = F(65535.0) / F(white)
    for frame in frames:
        h, w = frame.shape
        for ty in range(h // 16):
            for tx in range(w // 16):
                for p in range(4):
                    k = (pattern >> (2 * p)) & 3
                    q, bad = [[0] * 8 for _ in range(8)], False
                    for r in range(8):
                        for c in range(8):
                            x = F(frame[16 * ty + 2 * r + (p >> 1), 16 * tx + 2 * c + (p & 1)])
                            if math.isnan(x):
                                bad = True
                                continue
                            t = F(x * scale)
                            q[r][c] = int(np.rint(min(max(t, F(0)), F(65535))))
                    counters[0, k] += 1
                    if bad:
                        counters[1, k] += 1
                        continue
                    flat = [v for row in q for v in row]
                    if min(flat) < clip[0] or max(flat) > clip[1]:
                        counters[2, k] += 1
                        continue
                    e = sum((2 * q[r][c] - q[r][c - 1] - q[r][c + 1]) ** 2 for r in range(8) for c in range(1, 7))
                    e += sum((2 * q[r][c] - q[r - 1][c] - q[r + 1][c]) ** 2 for r in range(1, 7) for c in range(8))
                    i = ((sum(flat) // 64) * bins) // 65536
                    l = 0
                    while l + 1 < spec.LEVELS and spec.level_edge(l + 1) <= e:
                        l += 1
                    hist[k, i, l] += 1
                    sums[k, i] += sum(flat)
    return np.concatenate([hist.reshape(-1), sums.reshape(-1), counters.reshape(-1)])


def scene(rng, h, w, dtype=np.float32, white=1.0):
    yy, xx = np.mgrid[0:h, 0:w]
    v = (0.05 + 0.9 * xx / w * (0.4 + 0.6 * yy / h) + rng.normal(0, 0.01 + 0.02 * xx / w, (h, w))) * white
    if np.issubdtype(dtype, np.integer):
        return np.clip(np.rint(v), 0, 65535).astype(dtype)
    return v.astype(dtype)


@pytest.mark.parametrize('pattern', [spec.RGGB, spec.BGGR, spec.GRBG, spec.GBRG], ids=['RGGB', 'BGGR', 'GRBG', 'GBRG'])
def test_block_statistics_against_a_loop_over_sites(pattern):
    rng = np.random.default_rng(11)
    a = scene(rng, 50, 70)
    a[3, 5], a[20, 40], a[33, 2] = np.nan, np.inf, -np.inf
    a[40:44, 50:60] = 1.5
    b = scene(rng, 50, 70)
    for bins, white, clip in ((32, 1.0, (1, 64224)), (7, 0.9, (0, 65535)), (2, 1.7, (3000, 40000))):
        stats = spec.block_statistics([a, b], pattern, bins, white, clip)
        got = spec.counts_vector(stats)
        assert np.array_equal(got, brute_force([a, b], pattern, bins, white, clip)), (bins, white, clip)
        assert sum(stats['blocks']) == 2 * 4 * 3 * 4 and stats['blocks'][1] == 2 * stats['blocks'][0]
        assert sum(stats['nan']) == 1 and sum(stats['blocks']) == sum(stats['nan']) + sum(stats['clipped']) + sum(n for c in stats['hist'] for r in c for n in r)
    u = scene(rng, 32, 48, np.uint16, 65535.0)
    assert np.array_equal(spec.counts_vector(spec.block_statistics([u], pattern, 32, 65535.0, (1, 64224))), brute_force([u], pattern, 32, 65535.0, (1, 64224)))
    q, _ = spec.quantise(u, 65535.0)
    assert np.array_equal(q, u.astype(np.int64))   # uint16 storage with white = 65535 is exact
    small = spec.block_statistics([scene(rng, 14, 18)], pattern)
    assert not spec.counts_vector(small).any()


# ------------------------------------------------------------------ the median and the fit
def test_bin_point_is_the_median_level():
    h = [0] * spec.LEVELS
    h[40], h[41], h[42] = 10, 20, 10
    x, v, w = spec.bin_point(h, 40 * 64 * 1000, 1.0, 16)
    lo, hi = spec.level_edge(41), spec.level_edge(42)
    assert v == ((lo + (20 - 10) / 20 * (hi - lo)) / (576.0 * spec.KAPPA)) * (1.0 / 65535.0) ** 2
    assert x == 1000 / 65535.0 and w == 40 / (v * v)
    assert spec.bin_point(h, 1, 1.0, 41) is None   # below min_count
    zero = [0] * spec.LEVELS
    zero[0] = 100
    top = [0] * spec.LEVELS
    top[127] = 100
    assert spec.bin_point(zero, 1, 1.0, 16) is None and spec.bin_point(top, 1, 1.0, 16) is None
    one = [0] * spec.LEVELS
    one[9] = 1
    assert spec.bin_point(one, 64, 2.0, 1)[1] == ((spec.level_edge(9) + 1.0 * (spec.level_edge(10) - spec.level_edge(9))) / (576.0 * spec.KAPPA)) * (2.0 / 65535.0) ** 2


def test_fit_against_polyfit_and_the_fallbacks():
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = int(rng.integers(2, 32))
        x = np.sort(rng.uniform(0.01, 0.9, n))
        v = (2e-4 * x + 3e-5) * rng.normal(1.0, 0.03, n)
        w = rng.integers(16, 2000, n) / v ** 2
        a, b, valid = spec.fit(list(zip(x.tolist(), v.tolist(), w.tolist())))
        pa, pb = np.polyfit(x, v, 1, w=np.sqrt(w))
        assert pa > 0 and pb > 0   # (the data keep clear of the fallbacks, which have their own cases below)
        assert valid == 1 and abs(a - pa) <= 1e-7 * abs(pa) and abs(b - pb) <= 1e-7 * abs(pb), (a, pa, b, pb)
    # a falling line: a = 0, b the weighted mean
    a, b, valid = spec.fit([(0.1, 3e-5, 4.0), (0.5, 2e-5, 1.0), (0.9, 1e-5, 3.0)])
    assert (a, valid) == (0.0, 1) and b == (4.0 * 3e-5 + 1.0 * 2e-5 + 3.0 * 1e-5) / 8.0
    # a line through a negative intercept: b = 0, a the slope through the origin
    pts = [(0.2, 1e-5, 2.0), (0.4, 5e-5, 1.0), (0.8, 13e-5, 1.5)]
    a, b, valid = spec.fit(pts)
    assert (b, valid) == (0.0, 1) and a == sum((w * x) * v for x, v, w in pts) / sum((w * x) * x for x, v, w in pts)
    # nothing to fit
    assert spec.fit([]) == (0.0, 0.0, 0) and spec.fit([(0.3, 1e-5, 9.0)]) == (0.0, 0.0, 0)
    assert spec.fit([(0.25, 1e-5, 8.0), (0.25, 2e-5, 4.0)]) == (0.0, 0.0, 0)   # one abscissa: the determinant is 12 * 0.75 - 3 * 3 = 0


# ------------------------------------------------------------------ the transform
MODEL = np.array([[2e-4, 1e-6, 1, 20], [5e-5, 4e-6, 1, 20], [1e-3, 1e-5, 1, 20]], F)


def test_transform_against_float64_formulas():
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.01, 1.2, (40, 52)).astype(F)
    gains = np.array([1.9, 1.0, 1.4], F)
    for pattern, shape in ((spec.GRBG, (40, 52)), (None, (40, 52, 1)), (None, (16, 43, 3))):
        for g in (None, gains):
            for s in (1.0, 0.05):
                v = x.reshape(-1)[:int(np.prod(shape))].reshape(shape)
                row = spec.rows_of(shape, pattern)
                gg = np.ones(3) if g is None else g.astype(np.float64)
                a = (gg * MODEL[:, 0].astype(np.float64))[row]
                b = (gg * gg * MODEL[:, 1].astype(np.float64))[row]
                y = spec.stabilize(v, MODEL, pattern, g, s)
                assert y.dtype == F and y.shape == shape
                want = 2 * s / a * np.sqrt(np.maximum(a * v.astype(np.float64) + 0.375 * a * a + b, 0))
                assert np.allclose(y, want, rtol=2e-6, atol=1e-6)
                back = spec.unstabilize(y, MODEL, pattern, g, s, 'algebraic')
                inside = a * v + 0.375 * a * a + b > 0
                assert np.abs(back - v)[inside].max() <= 2e-5   # the algebraic inverse returns the input
                d = np.maximum(y.astype(np.float64) / s, math.sqrt(1.5))
                closed = a * np.maximum(d * d / 4 + math.sqrt(1.5) / 4 / d - 11 / 8 / d ** 2 + 5 / 8 * math.sqrt(1.5) / d ** 3 - 1 / 8 - b / (a * a), 0)
                got = spec.unstabilize(y, MODEL, pattern, g, s, 'unbiased')
                assert np.allclose(got, closed, rtol=1e-4, atol=2e-6)
    # float16 on either side rounds once
    y16 = spec.stabilize(x.astype(np.float16), MODEL, spec.RGGB, None, 1.0, np.float16)
    assert y16.dtype == np.float16 and np.array_equal(y16, spec.stabilize(x.astype(np.float16).astype(F), MODEL, spec.RGGB).astype(np.float16))
    assert spec.unstabilize(y16, MODEL, spec.RGGB).dtype == np.float16


def test_the_unbiased_inverse_is_zero_at_its_lower_end_and_unbiased():
    model = np.array([[1.0, 0.0, 1, 2]] * 3, F)   # pure Poisson counts
    d = np.array([[0.0], [1.0], [math.sqrt(1.5)]], F)
    assert np.abs(spec.unstabilize(d, model)).max() < 1e-6
    rng = np.random.default_rng(2)
    for lam in (2.0, 10.0, 100.0):
        counts = rng.poisson(lam, 400000).astype(F).reshape(-1, 1)
        mean_y = float(spec.stabilize(counts, model).astype(np.float64).mean())
        x = float(spec.unstabilize(np.array([[mean_y]], F), model)[0, 0])
        assert abs(x - lam) <= 0.01 * lam + 0.02, (lam, x)   # E[f(z)] -> lambda, up to the error of the closed form and of the sample mean


def test_degenerate_branches_are_exact_inverses():
    rng = np.random.default_rng(4)
    x = rng.uniform(-0.1, 1.1, (12, 10, 3)).astype(F)
    model = np.array([[0.0, 4e-4, 1, 5], [2e-4, 1e-6, 0, 1], [0.0, 0.0, 1, 3]], F)   # Gaussian, invalid, nothing known
    y = spec.stabilize(x, model, sigma_out=0.5)
    assert np.array_equal(y[..., 0], (F(0.5) * x[..., 0]) / np.sqrt(F(4e-4)))
    assert np.array_equal(y[..., 1].view(np.int32), x[..., 1].view(np.int32)) and np.array_equal(y[..., 2].view(np.int32), x[..., 2].view(np.int32))
    assert abs(float(np.std(y[..., 0] - (x[..., 0] * 25.0)))) < 1e-5
    for inverse in ('unbiased', 'algebraic'):
        back = spec.unstabilize(y, model, sigma_out=0.5, inverse=inverse)
        assert np.array_equal(back[..., 0], (y[..., 0] / F(0.5)) * np.sqrt(F(4e-4))) and np.allclose(back[..., 0], x[..., 0], rtol=0, atol=3e-7)
        assert np.array_equal(back[..., 1:].view(np.int32), x[..., 1:].view(np.int32))
    nan = np.array([[np.nan, 1.0, np.inf]], F).reshape(1, 3, 1)
    out = spec.stabilize(nan, MODEL)
    assert out[0, 0, 0] == 0.0 and np.isinf(out[0, 2, 0])   # fmaxf of a NaN and 0 is 0


# ------------------------------------------------------------------ the accuracy chart
def chart(a, b, seed, h=512, w=768):
    rng = np.random.default_rng(seed)
    levels = np.geomspace(0.01, 0.9, 64).reshape(8, 8)
    clean = np.kron(levels, np.ones((h // 8, w // 8)))
    i, j = np.indices((h, w))
    clean = clean * np.array(CFA)[2 * (i & 1) + (j & 1)]
    noisy = clean + rng.normal(0.0, 1.0, (h, w)) * np.sqrt(a * clean + b)
    return (np.clip(np.rint(noisy * 65535.0), 0, 65535) / 65535.0).astype(F)


@pytest.fixture(scope='module')
def chart_fits():
    out = {}
    for a, b in CASES + [(0.0, 1e-4)]:
        for seed in range(3):
            frame = chart(a, b, seed)
            _, model, curve = spec.estimate([frame], spec.RGGB, min_count=16)
            out[(a, b, seed)] = (frame, model, curve)
    return out


def test_accuracy_chart_slope(chart_fits):
    worst = 0.0
    for (a, b, seed), (_, model, _) in chart_fits.items():
        if a == 0.0:
            continue
        assert (model[:, 2] == 1).all() and (model[:, 3] >= 2).all(), (a, b, seed, model)
        err = np.abs(model[:, 0].astype(np.float64) / a - 1.0)
        print(f'a={a:g} b={b:g} seed={seed}: a/true {(model[:, 0] / a).round(4).tolist()}, b/true {(model[:, 1] / b).round(3).tolist()}, bins {model[:, 3].tolist()}')
        worst = max(worst, float(err.max()))
    print(f'worst error of a over the 27 fits: {100 * worst:.2f} %')
    assert worst <= 0.06


def test_accuracy_chart_stabilised_green_is_flat(chart_fits):
    worst = 0.0
    for (a, b, seed), (frame, model, _) in chart_fits.items():
        if a == 0.0:
            continue
        for sigma_out in (1.0, 0.25) if seed == 0 else (1.0,):
            y = spec.stabilize(frame, model, spec.RGGB, None, sigma_out).astype(np.float64)
            green = y[0::2, 1::2]   # RGGB: CFA position 1
            sd = green.reshape(8, green.shape[0] // 8, 8, green.shape[1] // 8).std(axis=(1, 3))
            err = abs(float(sd.mean()) / sigma_out - 1.0)
            print(f'a={a:g} b={b:g} seed={seed} sigma_out={sigma_out}: mean sd of the stabilised green patches / sigma_out = {sd.mean() / sigma_out:.4f}')
            worst = max(worst, err)
    print(f'worst deviation: {100 * worst:.2f} %')
    assert worst <= 0.03


def test_accuracy_chart_pure_read_noise(chart_fits):
    for (a, b, seed), (_, model, _) in chart_fits.items():
        if a != 0.0:
            continue
        print(f'a=0 b={b:g} seed={seed}: a {model[:, 0].tolist()}, b/true {(model[:, 1] / b).round(4).tolist()}')
        assert (model[:, 2] == 1).all()
        assert (np.abs(model[:, 0]) < 1e-5).all() and (np.abs(model[:, 1].astype(np.float64) / b - 1.0) <= 0.03).all()


def test_median_factor_is_what_the_constants_script_derives():
    """profiles/noiseprofile_constants.py at a tenth of its sample: the median of E / (576 s^2) for white Gaussian noise."""
    import importlib.util
    from pathlib import Path

    path = Path(__file__).resolve().parent.parent / 'profiles' / 'noiseprofile_constants.py'
    mod_spec = importlib.util.spec_from_file_location('noiseprofile_constants', path)
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    median, mean = mod.median_factor(blocks=400000, seed=7)
    assert abs(median - spec.KAPPA) < 3 * 1.5e-4 * math.sqrt(10) and abs(mean - 1.0) < 2e-3   # three standard errors at this sample
