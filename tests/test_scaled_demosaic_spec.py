"""CPU-only: the float32 restatement of the reduced-size demosaic (tests/scaled_demosaic_spec.py, include/tdk_hip_scaled.h) held to

  * literal per-output loops in exact rational arithmetic with one rounding per written operation, on tiny frames;
  * the tap rule: every output has a tap of each parity on each axis, at most 32 taps, for every (n_in, n_out) with n_in <= 80;
  * the header's identities: pattern swap, flat frames within the derived bound, fused equals unfused;
  * what the stage is for: on a supersampled scene its chroma error at achromatic edges and its error to the area-averaged truth are
    below those of 2 x 2 binning followed by the scaler, at ratios 2 and 4; the error beside the oracle's RCD followed by the scaler
    is printed, not asserted;
  * a special sample: an inf or a NaN at one site reaches exactly the outputs whose footprint of that colour holds the site.

Purpose test, measured on the restatement (RGGB, 256 x 256 mosaic; chroma = RMS of R-G and B-G over the achromatic half, error = RMS
to the area average of the supersampled scene; 'binning' is 2 x 2 binning followed by the scaler's float64 restatement, 'rcd' the
oracle's RCD followed by it):

    noise  ratio   chroma: this  binning     error: this  binning  rcd      this/binning
    no     2       0.0931        0.2417      0.0722       0.1223   0.0627   0.59
    no     3       0.0666        0.1062      0.0545       0.0776   0.0495   0.70
    no     4       0.0497        0.0698      0.0525       0.0690   0.0508   0.76
    yes    2       0.0938        0.2422      0.0725       0.1228   0.0628   0.59
    yes    3       0.0672        0.1064      0.0547       0.0778   0.0496   0.70
    yes    4       0.0502        0.0701      0.0526       0.0691   0.0510   0.76

(The scene is harsh on purpose: hard bars 4.85 sites wide, a chirp and a checker of 3-site squares, all close to the mosaic's Nyquist
limit.  RCD followed by the scaler stays a little closer to the truth than the area average -- it costs a 12 MP demosaic.)
"""
from fractions import Fraction

import numpy as np
import pytest

import scaled_demosaic_spec as spec
from test_resample_spec import resize_ref

f32 = np.float32
TINY = [((2, 2), (1, 1)), ((3, 3), (1, 1)), ((7, 5), (3, 2)), ((37, 22), (13, 9))]   # (W, H) -> (w, h)


# ---- exact arithmetic, one rounding per operation: shares nothing with the restatement's float64 tricks
def rnd(q: Fraction) -> Fraction:
    """q rounded to the nearest float32 value, ties to even (normal and subnormal range; the tests stay far from overflow)."""
    if q == 0:
        return Fraction(0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** max(e - 23, -149)
    n, rest = divmod(a, ulp)
    if rest * 2 > ulp or (rest * 2 == ulp and n % 2 == 1):
        n += 1
    return sign * n * ulp


def literal(x, ow, oh, pattern):
    """Every output on its own, straight from the header's text."""
    h, w = x.shape
    X = [[Fraction(float(v)) for v in row] for row in x]

    def taps(i, n_in, n_out):
        found = []
        for j in range(n_in):
            num = 2 * n_out * j + n_out - (2 * i + 1) * n_in
            if abs(num) < 2 * n_in:
                found.append((j, rnd(1 - rnd(Fraction(abs(num), 2 * n_in)))))
        return found

    def chain(terms):
        acc = total = None
        for wt, v in terms:
            acc = rnd(wt * v) if acc is None else rnd(wt * v + acc)
            total = wt if total is None else rnd(total + wt)
        return acc, total

    out = np.zeros((oh, ow, 3), f32)
    for o in range(oh):
        ty = taps(o, h, oh)
        for i in range(ow):
            tx = taps(i, w, ow)
            B, Sy, Sx = {}, {}, {}
            for p in (0, 1):
                Sx[p] = chain([(wt, Fraction(0)) for j, wt in tx if j & 1 == p])[1]
                for q in (0, 1):
                    rows = [(v, chain([(wt, X[y][j]) for j, wt in tx if j & 1 == p])[0]) for y, v in ty if y & 1 == q]
                    B[q, p], Sy[q] = chain(rows)
            sites = {c: [(q, p) for q in (0, 1) for p in (0, 1) if spec.cfa_color(q, p, pattern) == c] for c in (0, 1, 2)}
            for c in (0, 2):
                (q, p), = sites[c]
                out[o, i, c] = float(rnd(B[q, p] / rnd(Sy[q] * Sx[p])))
            (q1, p1), (q2, p2) = sites[1]
            assert q1 == 0 and q2 == 1
            den = rnd(rnd(Sy[q1] * Sx[p1]) + rnd(Sy[q2] * Sx[p2]))
            out[o, i, 1] = float(rnd(rnd(B[q1, p1] + B[q2, p2]) / den))
    return out


def test_fmaf_is_one_rounding():
    rng = np.random.default_rng(11)
    a, b = rng.random(4000, dtype=f32), rng.random(4000, dtype=f32)
    c = (rng.random(4000, dtype=f32) - f32(0.5)) * f32(2.0) ** rng.integers(-30, 4, 4000).astype(f32)
    got = spec.fmaf(a, b, c)
    want = np.array([float(rnd(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))) for x, y, z in zip(a, b, c)], dtype=f32)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a case float64 rounds twice: the product's low bits decide a tie of the sum
    x, y, z = f32(1 + 2.0 ** -23), f32(1 + 2.0 ** -23), f32(2.0 ** 24)
    assert float(spec.fmaf(x, y, z)) == float(rnd(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))) == 2.0 ** 24 + 2.0
    assert np.isnan(spec.fmaf(f32(np.nan), f32(1), f32(1))) and np.isinf(spec.fmaf(f32(np.inf), f32(1), f32(1)))


@pytest.mark.parametrize('src,dst', TINY)
@pytest.mark.parametrize('name', ['RGGB', 'GBRG'])
def test_restatement_is_the_literal_loops(src, dst, name):
    rng = np.random.default_rng(src[0] * 100 + dst[0])
    x = (rng.random((src[1], src[0]), dtype=f32) * f32(1.5)).astype(f32)
    got = spec.scaled_demosaic(x, dst[0], dst[1], spec.PATTERNS[name])
    want = literal(x, dst[0], dst[1], spec.PATTERNS[name])
    assert got.shape == (dst[1], dst[0], 3) and got.dtype == f32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_every_output_has_a_tap_of_each_parity_and_at_most_32():
    cases = 0
    for n_out in range(1, 41):
        for n_in in range(2 * n_out, min(16 * n_out, 80) + 1):
            for i, (j, w) in enumerate(spec.axis_taps(n_in, n_out)):
                assert len(j) <= spec.MAX_TAPS and (j & 1 == 0).any() and (j & 1 == 1).any(), (n_in, n_out, i)
                assert (np.diff(j) == 1).all() and (w > 0).all() and (w <= 1).all() and j[0] >= 0 and j[-1] < n_in
                num = 2 * n_out * j + n_out - (2 * i + 1) * n_in   # and nothing outside takes part
                assert (np.abs(num) < 2 * n_in).all()
                for outside in (j[0] - 1, j[-1] + 1):
                    assert not 0 <= outside < n_in or abs(2 * n_out * outside + n_out - (2 * i + 1) * n_in) >= 2 * n_in
            cases += 1
    assert cases > 1000
    for n_in, n_out in ((2, 1), (3, 1), (5, 2), (7, 3), (37, 13), (33, 16), (17, 8), (64, 4)):   # the pairs the header names
        assert all((j & 1 == 0).any() and (j & 1 == 1).any() for j, _ in spec.axis_taps(n_in, n_out))
    assert max(len(j) for j, _ in spec.axis_taps(64, 4)) == 32 and max(len(j) for j, _ in spec.axis_taps(65535 // 4096 * 4096, 4096)) <= 32


def test_pattern_swap_identity():
    rng = np.random.default_rng(3)
    x = rng.random((22, 37), dtype=f32)
    for a, b in (('RGGB', 'BGGR'), ('GRBG', 'GBRG')):
        u, v = spec.scaled_demosaic(x, 13, 9, spec.PATTERNS[a]), spec.scaled_demosaic(x, 13, 9, spec.PATTERNS[b])
        assert np.array_equal(u[..., 0].view(np.uint32), v[..., 2].view(np.uint32)) and np.array_equal(u[..., 2].view(np.uint32), v[..., 0].view(np.uint32))
        assert np.array_equal(u[..., 1].view(np.uint32), v[..., 1].view(np.uint32))
    assert not np.array_equal(spec.scaled_demosaic(x, 13, 9, spec.RGGB), spec.scaled_demosaic(x, 13, 9, spec.GRBG))


@pytest.mark.parametrize('src,dst', TINY + [((64, 32), (4, 2)), ((33, 17), (16, 8)), ((80, 60), (27, 7))])
def test_flat_frames_come_back_within_the_derived_bound(src, dst):
    colours = np.array([0.8131, 0.3377, 1.6021], dtype=f32)   # above 1 too: nothing clamps without gains
    bound = spec.flat_bound(src[0], src[1], dst[0], dst[1])
    assert bound < 2 * (32 + 32 + 1) * 2.0 ** -24 * 1.001
    for name, pattern in spec.PATTERNS.items():
        yy, xx = np.mgrid[0:src[1], 0:src[0]]
        out = spec.scaled_demosaic(colours[spec.cfa_color(yy, xx, pattern)], dst[0], dst[1], pattern).astype(np.float64)
        rel = np.abs(out / colours.astype(np.float64) - 1.0).max()
        print(f'{src} -> {dst} {name}: flat-frame error {rel:.3e}, bound {bound:.3e}')
        assert rel <= bound, (name, rel, bound)


def test_fused_forms_are_the_two_step_forms():
    rng = np.random.default_rng(8)
    codes = rng.integers(0, 4096, (22, 38))
    gains = np.array([1.9, 1.0, 1.6], dtype=f32)
    for ids in (False, True):
        packed = spec.encode12(codes, ids)
        x = spec.decode12(packed, 38, 22, ids)
        assert np.array_equal(x, codes.astype(f32) * (f32(1) / f32(4095)))
        two_step = spec.scaled_demosaic(spec.balance(x, gains, spec.GRBG), 13, 9, spec.GRBG)
        assert np.array_equal(spec.scaled_demosaic(x, 13, 9, spec.GRBG, gains=gains).view(np.uint32), two_step.view(np.uint32))
    assert (x * gains.max() > 1).any() and spec.balance(x, gains, spec.GRBG).max() == 1.0   # the clamp takes part
    half = x.astype(np.float16).astype(f32)
    stored = spec.balance(half, gains, spec.GRBG, half=True)
    assert np.array_equal(stored, stored.astype(np.float16).astype(f32))
    assert np.array_equal(spec.scaled_demosaic(half, 13, 9, spec.GRBG, gains=gains, half_source=True), spec.scaled_demosaic(stored, 13, 9, spec.GRBG))
    assert spec.balance(np.array([[np.nan, np.inf], [-np.inf, 0.5]], dtype=f32), gains, spec.RGGB).tolist() == [[0.0, 1.0], [0.0, 0.800000011920929]]


@pytest.mark.parametrize('bad', [np.inf, -np.inf, np.nan])
def test_a_special_sample_reaches_exactly_its_footprint(bad):
    rng = np.random.default_rng(21)
    w, h, ow, oh = 37, 22, 13, 9
    x = rng.random((h, w), dtype=f32)
    clean = spec.scaled_demosaic(x, ow, oh, spec.RGGB)
    xt, yt = spec.axis_taps(w, ow), spec.axis_taps(h, oh)
    for sy, sx in ((0, 0), (7, 12), (8, 13), (21, 36), (10, 5)):
        y = x.copy()
        y[sy, sx] = bad
        out = spec.scaled_demosaic(y, ow, oh, spec.RGGB)
        c = spec.cfa_color(sy, sx, spec.RGGB)
        hit = np.zeros((oh, ow, 3), bool)
        hit[np.ix_([o for o in range(oh) if sy in yt[o][0]], [i for i in range(ow) if sx in xt[i][0]], [c])] = True
        assert hit.any() and not hit.all()
        assert not np.isfinite(out[hit]).any() and np.array_equal(out[~hit].view(np.uint32), clean[~hit].view(np.uint32))
        if not np.isnan(bad):
            assert (out[hit] == bad).all()


# ---- what the stage is for
def scene(n=256, ss=4):
    """(n*ss, n*ss, 3) float64: the left half achromatic -- slanted bars, a radial chirp, a checker of 3-site squares -- the right half
    tinted patches with soft and hard borders."""
    yy, xx = (np.mgrid[0:n * ss, 0:n * ss] + 0.5) / ss
    half = n // 2
    bars = 0.5 + 0.45 * np.sign(np.sin(2 * np.pi * (xx + 0.31 * yy) / 9.7))
    r2 = (xx - half / 2) ** 2 + (yy - n * 0.5) ** 2
    chirp = 0.5 + 0.4 * np.cos(r2 / 90.0)
    checker = 0.15 + 0.7 * ((np.floor(xx / 3) + np.floor(yy / 3)) % 2)
    grey = np.where(yy < n / 3, bars, np.where(yy < 2 * n / 3, chirp, checker))
    img = np.repeat(grey[..., None], 3, axis=2)
    tints = np.array([[0.9, 0.3, 0.2], [0.2, 0.7, 0.3], [0.25, 0.3, 0.85], [0.8, 0.75, 0.2], [0.6, 0.2, 0.7], [0.1, 0.6, 0.65]])
    patch = (np.floor((xx - half) / (half / 3)).astype(int).clip(0, 2) + 3 * np.floor(yy / (n / 2)).astype(int).clip(0, 1))
    shade = 0.55 + 0.45 * np.sin(2 * np.pi * yy / 61.0) * np.cos(2 * np.pi * xx / 47.0)
    right = tints[patch] * shade[..., None]
    img[:, half * ss:] = right[:, half * ss:]
    return img


def area_average(img, n_out, axis):
    """Box average of axis `axis` onto n_out equal cells, fractional coverage included, float64."""
    n_in = img.shape[axis]
    edges = np.arange(n_out + 1) * (n_in / n_out)
    lo, hi = np.arange(n_in)[None, :], np.arange(n_in)[None, :] + 1
    cover = np.clip(np.minimum(hi, edges[1:, None]) - np.maximum(lo, edges[:-1, None]), 0, None)
    cover /= cover.sum(1, keepdims=True)
    return np.moveaxis(np.tensordot(cover, np.moveaxis(img, axis, 0), axes=1), 0, axis)


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


@pytest.fixture(scope='module')
def purpose(oracle):
    """{(noisy, ratio): figures} on one scene, computed once."""
    n, ss = 256, 4
    fine = scene(n, ss)
    full = area_average(area_average(fine, n, 0), n, 1)
    yy, xx = np.mgrid[0:n, 0:n]
    clean = full[yy, xx, spec.cfa_color(yy, xx, spec.RGGB)]
    rng = np.random.default_rng(2024)
    noisy = clean + rng.standard_normal(clean.shape) * np.sqrt(4e-4 * clean + 1e-5)
    out = {}
    for is_noisy, mosaic in ((False, clean), (True, noisy)):
        mosaic = mosaic.astype(f32)
        binned = spec.bin2x2(mosaic, spec.RGGB)
        rcd = oracle.rcd(mosaic, spec.RGGB).astype(np.float64)
        for ratio in (2, 3, 4):
            m = n // ratio
            truth = area_average(area_average(fine, m, 0), m, 1)
            grey = slice(0, int(np.floor((n // 2 - 4) / (n / m))))   # the output columns wholly inside the achromatic half
            this = spec.scaled_demosaic(mosaic, m, m, spec.RGGB).astype(np.float64)
            other = resize_ref(binned, m, m)
            demosaiced = resize_ref(rcd, m, m)

            def chroma(v):
                return rms(np.stack([v[:, grey, 0] - v[:, grey, 1], v[:, grey, 2] - v[:, grey, 1]]))

            out[is_noisy, ratio] = dict(chroma=chroma(this), chroma_binning=chroma(other), error=rms(this - truth), error_binning=rms(other - truth),
                                        error_rcd=rms(demosaiced - truth))
    return out


@pytest.mark.parametrize('noisy', [False, True])
@pytest.mark.parametrize('ratio', [2, 3, 4])
def test_registered_average_beats_binning(purpose, noisy, ratio):
    f = purpose[noisy, ratio]
    print(f"noise {'yes' if noisy else 'no'} ratio {ratio}: chroma {f['chroma']:.4f} (binning {f['chroma_binning']:.4f}); error to the area average "
          f"{f['error']:.4f} (binning {f['error_binning']:.4f}, oracle RCD + scaler {f['error_rcd']:.4f}); this / binning {f['error'] / f['error_binning']:.2f}")
    if ratio in (2, 4):
        assert f['chroma'] < f['chroma_binning']
        assert f['error'] < f['error_binning']
