"""CPU-only: the NumPy restatement tests/filmic_spec.py of include/tdk_hip_filmic.h against literal per-pixel loops, the identities
the header states, and the purpose of the stage: the curve torch_darktable.Filmic builds runs through black, grey and white, is
monotone and has the contrast asked for; hue survives the curve under the 'max' norm; white is reached achromatically; no value leaves
the display range; and the tables interpolate the analytic curve and encoding to a quarter of a uint8 step."""

import math

import numpy as np
import pytest
import torch

import filmic_spec as spec

F = np.float32
CUDA = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one


def literal_pixel(x, T, D, G, e, norm, w):
    """One pixel by the header's text, scalar float32 operations."""
    def pos(v):
        return v if v > 0 else F(0.0)

    def index(c, ev_min):
        b = int(np.array(c, dtype=F).view(np.uint32))
        ex, M = (b >> 23) - 127, b & 0x7FFFFF
        return (ex - ev_min) * 32 + (M >> 18), F(M & 0x3FFFF) / F(262144.0)

    def look(table, c, ev_min):
        i, f = index(c, ev_min)
        return table[i] + f * (table[i + 1] - table[i])

    def clamp(N):
        return np.fmin(np.fmax(N, spec.XMIN), spec.XMAX)

    with np.errstate(all='ignore'):
        p = [np.fmin(pos(F(v) * F(e)), spec.XMAX) for v in x]
        if norm == spec.NONE:
            o = [look(T, clamp(c), -20) for c in p]
        else:
            if norm == spec.MAX:
                N = np.fmax(np.fmax(p[0], p[1]), p[2])
            elif norm == spec.LUMA:
                N = (F(w[0]) * p[0] + F(w[1]) * p[1]) + F(w[2]) * p[2]
            else:
                q = [c * c for c in p]
                k = [q[c] * p[c] for c in range(3)]
                den, num = (q[0] + q[1]) + q[2], (k[0] + k[1]) + k[2]
                N = num / den if den > 0 else F(0.0)
            Nc = clamp(N)
            y, d = look(T, Nc, -20), look(D, Nc, -20)
            o = [y * (F(1.0) + d * (c / Nc - F(1.0))) for c in p]
            m = np.fmax(np.fmax(o[0], o[1]), o[2])
            if m > 1:
                if y >= 1:
                    o = [F(1.0)] * 3
                else:
                    g = (F(1.0) - y) / (m - y)
                    o = [y + (c - y) * g for c in o]
        if G is None:
            return o
        v = []
        for c in o:
            oc = np.fmin(pos(c), spec.BELOW_ONE)
            v.append((oc * F(65536.0)) * G[0] if oc < spec.ENC_LO else look(G, oc, -16))
        return v


def tables(f):
    return f.host_curve.numpy(), None if f.host_encode is None else f.host_encode.numpy()


@pytest.mark.parametrize('norm', ['max', 'luma', 'power', 'none'])
def test_the_restatement_matches_literal_loops(td, norm):
    x = spec.samples(700, np.float32, seed=3)
    half = spec.samples(700, np.float16, seed=4)
    for f, e in ((td.Filmic(CUDA, norm=norm), 1.0), (td.Filmic.sigmoid(CUDA, norm=norm, encoding=None), 2.5), (td.Filmic(CUDA, norm=norm, encoding='gamma:2.2'), 0.3)):
        curve, G = tables(f)
        for source in (x, half):
            got = spec.filmic(source, curve, G, e, spec.NORMS[norm], f.weights)
            expected = np.array([literal_pixel(px, curve[0], curve[1], G, e, spec.NORMS[norm], f.weights) for px in source.astype(F)], dtype=F)
            assert got.dtype == F and np.array_equal(got.view(np.uint32), expected.view(np.uint32)), (norm, f, source.dtype)
            with np.errstate(over='ignore', invalid='ignore'):
                assert np.array_equal(spec.filmic(source, curve, G, e, spec.NORMS[norm], f.weights, np.float16).view(np.uint16), expected.astype(np.float16).view(np.uint16))
                codes = np.rint(np.fmin(np.fmax(expected, F(0)), F(1)) * F(255)).astype(np.uint8)
            assert np.array_equal(spec.filmic(source, curve, G, e, spec.NORMS[norm], f.weights, np.uint8), codes)


def test_constants_and_nodes(td):
    from torch_darktable import _native

    assert (spec.EV_MIN, spec.EV_MAX, spec.STEPS, spec.TABLE, spec.ENC_EV_MIN, spec.ENC_TABLE) == (-20, 12, 32, 1025, -16, 513)
    assert (_native.TDK_FILMIC_EV_MIN, _native.TDK_FILMIC_EV_MAX, _native.TDK_FILMIC_STEPS, _native.TDK_FILMIC_TABLE) == (-20, 12, 32, 1025)
    assert (_native.TDK_FILMIC_ENC_EV_MIN, _native.TDK_FILMIC_ENC_TABLE) == (-16, 513)
    assert (_native.TDK_FILMIC_MAX, _native.TDK_FILMIC_LUMA, _native.TDK_FILMIC_POWER, _native.TDK_FILMIC_NONE) == (spec.MAX, spec.LUMA, spec.POWER, spec.NONE) == (0, 1, 2, 3)
    assert float(spec.XMIN) == 2.0 ** -20 and float(spec.XMAX) == 4096.0 - 2.0 ** -12 and float(spec.BELOW_ONE) == 1.0 - 2.0 ** -24
    nodes = td.Filmic.table_nodes()
    assert nodes.dtype == torch.float64 and nodes.shape == (1025,) and np.array_equal(nodes.numpy(), spec.nodes())
    assert nodes[0] == 2.0 ** -20 and nodes[1024] == 4096.0 and nodes[640] == 1.0 and nodes[33] == (1 + 1 / 32) * 2.0 ** -19
    assert np.array_equal(nodes.numpy().astype(F).astype(np.float64), nodes.numpy())   # every node is a float32
    enc = td.Filmic.encoding_nodes()
    assert enc.shape == (513,) and enc[0] == 2.0 ** -16 and enc[512] == 1.0 and np.array_equal(enc.numpy(), spec.nodes(-16, 513))
    # a value's index is the last node at or below it
    x = np.exp2(np.random.default_rng(0).uniform(-20, 12, 5000)).astype(F)
    i, f = spec.index(x, -20)
    n = spec.nodes()
    assert (n[i] <= x).all() and (x < n[i + 1]).all() and np.allclose(n[i] + f.astype(np.float64) * (n[i + 1] - n[i]), x, rtol=0, atol=0)


def test_identities():
    """With T[j] the node's position, no encoding and e = 1, 'none' returns the source's bits on [XMIN, XMAX]; with G[512] = 1 the top
    code is 255."""
    n = spec.nodes().astype(F)
    curve = np.stack((n, np.ones_like(n)))
    rng = np.random.default_rng(1)
    x = np.exp2(rng.uniform(-20, 12, (200000, 3))).astype(F)
    x = np.concatenate((np.fmin(x, spec.XMAX), np.repeat(n[:-1, None], 3, 1), np.repeat(np.nextafter(n[1:, None], F(0)), 3, 1), [[spec.XMIN, spec.XMAX, F(1.0)]])).astype(F)
    out = spec.filmic(x, curve, None, 1.0, spec.NONE)
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32))
    # outside: clamped to the ends
    out = spec.filmic(np.array([[0.0, -1.0, np.nan], [np.inf, 5000.0, 2.0 ** -21]], dtype=F), curve, None, 1.0, spec.NONE)
    assert np.array_equal(out, np.array([[spec.XMIN] * 3, [spec.XMAX, spec.XMAX, spec.XMIN]], dtype=F))
    G = spec.nodes(-16, 513).astype(F)   # a linear encoding: G[512] = 1
    top = spec.filmic(np.array([[1.0, 1.0, 1.0], [4000.0, 2.0, 1.0]], dtype=F), curve, G, 1.0, spec.NONE)
    assert top.max() < 1.0 and np.array_equal(spec.filmic(np.array([[1.0, 1.0, 1.0], [4000.0, 2.0, 1.0]], dtype=F), curve, G, 1.0, spec.NONE, out_dtype=np.uint8),
                                              np.full((2, 3), 255, dtype=np.uint8))


def test_the_curve_runs_through_black_grey_and_white(td):
    from torch_darktable.filmic import filmic_curve, filmic_spline

    for kw in (dict(), dict(grey=0.12, black_ev=-7.0, white_ev=4.5, contrast=1.3, latitude=0.1, target=(0.002, 0.2, 0.95)), dict(contrast=1.0, latitude=0.0),
               dict(black_ev=-10.0, white_ev=6.0, contrast=1.4, latitude=0.2, output_power=4.0)):
        s = filmic_spline(**kw)
        grey, black, white = s['grey'], s['grey'] * 2.0 ** s['black_ev'], s['grey'] * 2.0 ** s['white_ev']
        T, D = filmic_curve(torch.tensor([black, grey, white, black / 4, white * 4], dtype=torch.float64), s)
        assert np.allclose(T.numpy(), [*s['target'], s['target'][0], s['target'][2]], rtol=1e-9, atol=1e-12), kw
        assert D[1] == 1.0 and D[2] == 1.0 - s['desaturate'][1] and D[0] == 1.0 - s['desaturate'][0]
        if 'output_power' not in kw:
            assert math.isclose(s['v_g'], s['t_g'], rel_tol=1e-12)   # grey sits on the diagonal
        # the slope of v = T^(1/p) over t at grey is the contrast
        h = 1e-6 * (s['white_ev'] - s['black_ev'])
        pair, _ = filmic_curve(torch.tensor([grey * 2.0 ** -h, grey * 2.0 ** h], dtype=torch.float64), s)
        v = pair.numpy() ** (1.0 / s['output_power'])
        # (a central difference over 2e-6 in t: with latitude 0 the two sides are cubics of different curvature, |v''| <= 6 * secant / h
        # each, so the difference is off by up to 1e-6 * |v''| / 2 -- below 1e-4 for every case here)
        assert math.isclose((v[1] - v[0]) / 2e-6, s['contrast'], rel_tol=1e-4), kw
        # monotone, in the analytic curve on a fine grid and in the float32 table
        fine, _ = filmic_curve(torch.tensor(np.exp2(np.linspace(-20, 12, 200001)), dtype=torch.float64), s)
        assert (np.diff(fine.numpy()) >= 0).all(), kw
        f = td.Filmic(CUDA, **kw)
        table = f.host_curve.numpy()
        assert table.shape == (2, 1025) and table.dtype == F and (np.diff(table[0]) >= 0).all() and table[0].min() >= 0 and table[0].max() <= 1
        assert (table[1] >= 0).all() and (table[1] <= 1).all()
        assert f.parameters == s


def test_parameters_that_would_swing_are_refused(td):
    for kw, message in ((dict(contrast=5.0), 'leaves the range'), (dict(contrast=2.9, latitude=0.05), 'swing'), (dict(target=(0.00015, 0.1845, 1.0)), 'swing'),
                        (dict(contrast=1.9, latitude=0.5), 'swing|leaves the range'), (dict(grey=0.0), 'grey must be'), (dict(black_ev=1.0), 'black_ev must be'),
                        (dict(white_ev=-1.0), 'black_ev must be'), (dict(contrast=0.0), 'contrast must be'), (dict(latitude=1.0), 'latitude must be'),
                        (dict(latitude=-0.1), 'latitude must be'), (dict(target=(0.0, 0.5, 0.4)), 'target must be'), (dict(target=(0.0, 0.2)), 'target must be'),
                        (dict(output_power=0.0), 'output_power must be'), (dict(desaturate=(0.0, 1.5)), 'desaturate must be'), (dict(grey=float('nan')), 'finite')):
        with pytest.raises(ValueError, match=message):
            td.Filmic(CUDA, **kw)
    f = td.Filmic(CUDA)
    before = f.host_curve.clone()
    with pytest.raises(ValueError, match='leaves the range'):
        f.set_curve(contrast=5.0)
    assert torch.equal(f.host_curve, before) and f.parameters['contrast'] == 1.5   # a refused change leaves the object as it was
    f.set_curve(contrast=1.2)
    assert f.parameters['contrast'] == 1.2 and not torch.equal(f.host_curve, before)
    assert math.isclose(f.parameters['white_ev'], math.log2(1 / 0.18))   # white_ev None stays the default under a change of another parameter


def test_hue_survives_under_the_max_norm(td):
    """Where D = 1 the result's channel ratios are the source's: s_c = 1 + (r_c - 1) is r_c to within 2^-24 (the rounding of r_c - 1
    for r_c < 1/2), and y * s_c and the two divisions add a relative 2^-23 each."""
    f = td.Filmic(CUDA, norm='max', encoding=None)
    curve, _ = tables(f)
    rng = np.random.default_rng(7)
    s = f.parameters
    hi = s['grey'] * 2.0 ** (s['black_ev'] + s['t_hi'] * (s['white_ev'] - s['black_ev']))   # D = 1 below the shoulder (no desaturation of shadows by default)
    level = np.exp2(rng.uniform(math.log2(s['grey']) - 6.0, math.log2(hi), (20000, 1)))
    x = (level * rng.uniform(0.05, 1.0, (20000, 3))).astype(F)
    x = x[(x.max(axis=-1) < hi * 0.999) & (x.max(axis=-1) > s['grey'] * 2.0 ** -6)]   # above black: the curve is not 0
    out = spec.filmic(x, curve, None, 1.0, spec.MAX).astype(np.float64)
    x = x.astype(np.float64)
    got, expected = out / out.max(axis=-1, keepdims=True), x / x.max(axis=-1, keepdims=True)
    assert len(x) > 10000 and np.abs(got - expected).max() <= 2.0 ** -24 + 3 * 2.0 ** -23
    assert (out.argmax(axis=-1) == x.argmax(axis=-1)).all()
    # ... and the per-channel curve does shift them
    plain = spec.filmic(x.astype(F), curve, None, 1.0, spec.NONE).astype(np.float64)
    assert np.abs(plain / plain.max(axis=-1, keepdims=True) - expected).max() > 0.1


def test_white_is_reached_achromatically(td):
    """A pixel whose norm is at white or above is (1, 1, 1) whatever its hue: y = 1 and D = 0 there."""
    hues = np.array([[1.0, 0.2, 0.05], [1.0, 1.0, 0.0], [0.3, 1.0, 0.9], [0.0, 0.0, 1.0], [0.6, 0.5, 0.4]])
    for f in (td.Filmic(CUDA, encoding=None), td.Filmic(CUDA, norm='luma', encoding=None), td.Filmic(CUDA, norm='power', encoding=None)):
        curve, _ = tables(f)
        norm_of = {'max': hues.max(axis=-1), 'luma': hues @ np.array(f.weights), 'power': (hues ** 3).sum(axis=-1) / (hues ** 2).sum(axis=-1)}[f.norm]
        for above in (1.001, 4.0, 3000.0):
            x = (hues * (above / norm_of)[:, None]).astype(F)
            assert np.array_equal(spec.filmic(x, curve, None, 1.0, spec.NORMS[f.norm], f.weights), np.ones_like(x)), (f.norm, above)
            assert np.array_equal(spec.filmic(x, curve, tables(td.Filmic(CUDA))[1], 1.0, spec.NORMS[f.norm], f.weights, out_dtype=np.uint8), np.full(x.shape, 255, dtype=np.uint8))
    # saturation goes smoothly: D falls from 1 at the end of the latitude to 0 at white
    D = td.Filmic(CUDA).host_curve.numpy()[1]
    n = spec.nodes()
    assert D[n <= 0.18].min() == 1.0 and D[n >= 1.0].max() == 0.0 and (np.diff(D[(n > 0.18) & (n < 1.0)]) <= 0).all()


@pytest.mark.parametrize('norm', ['luma', 'power'])
def test_a_saturated_ramp_stays_in_the_display_range(td, norm):
    """Fourteen stops of the six saturated hues and of pastel ones, also with all the saturation kept up to white (desaturate 0, where the
    gamut step has the most to do): no result leaves [0, 1]."""
    ramp = np.exp2(np.linspace(-10.0, 4.0, 3000))[:, None, None]
    hues = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 0.02, 0.02], [0.05, 0.05, 1], [1, 0.5, 0.0], [1, 0.7, 0.4]], dtype=np.float64)[None]
    x = (ramp * hues).reshape(-1, 3).astype(F)
    for f in (td.Filmic(CUDA, norm=norm), td.Filmic.sigmoid(CUDA, norm=norm), td.Filmic(CUDA, norm=norm, desaturate=(0.0, 0.0), encoding='gamma:2.2')):
        curve, G = tables(f)
        out, fires = spec.filmic(x, curve, G, 1.0, spec.NORMS[norm], f.weights, return_fires=True)
        if norm == 'luma' or f.parameters.get('desaturate') == (0.0, 0.0):   # blue is far above its luminance; the power norm is below the largest channel of a pastel hue
            assert fires.sum() > 500, fires.sum()
        assert out.min() >= 0.0 and out.max() <= 1.0 and np.isfinite(out).all(), (norm, f, out.min(), out.max())
        linear = spec.filmic(x, curve, None, 1.0, spec.NORMS[norm], f.weights)
        assert linear.min() >= 0.0 and linear.max() <= 1.0 + 2.0 ** -22   # in front of the encoding: to within the rounding of the pull


LIMIT = 1.0 / 1020.0   # a quarter of a uint8 step


@pytest.mark.parametrize('kind', ['filmic', 'sigmoid'])
def test_the_tables_interpolate_the_analytic_curve(td, kind):
    """The shipped defaults: table lerp of the curve, then table lerp of sRGB, against both in float64.  Measured:
    6.6e-5 for the filmic spline and 4.8e-5 for the sigmoid at 32 nodes per octave."""
    from torch_darktable.filmic import encoding_curve, filmic_curve, sigmoid_curve

    f = td.Filmic(CUDA) if kind == 'filmic' else td.Filmic.sigmoid(CUDA)
    curve, G = tables(f)
    grid = np.exp2(np.linspace(-21.0, 13.0, 400001))
    x = np.repeat(grid[:, None], 3, 1).astype(F)
    got = spec.filmic(x, curve, G, 1.0, spec.MAX)[:, 0].astype(np.float64)
    clamped = torch.tensor(np.clip(x[:, 0].astype(np.float64), 2.0 ** -20, float(spec.XMAX)))
    if kind == 'filmic':
        T, _ = filmic_curve(clamped, f.parameters)
    else:
        p = f.parameters
        T, _ = sigmoid_curve(clamped, p['grey'], p['contrast'], p['target_grey'], p['desaturate'], p['desaturate_ev'])
    expected = encoding_curve('srgb')(T.clamp(0.0, 1.0)).numpy()
    error = np.abs(got - expected).max()
    print(kind, 'largest error in display value', error)
    assert error <= LIMIT
    assert error < 1e-4   # ... and by a wide margin
    if kind == 'sigmoid':   # the curve itself: through (grey, target grey), rising
        y, _ = sigmoid_curve(torch.tensor([0.18, 0.09, 0.36], dtype=torch.float64), 0.18, 1.5, 0.1845, 1.0, (0.0, 6.0))
        assert math.isclose(float(y[0]), 0.1845, rel_tol=1e-12) and y[1] < y[0] < y[2]


def test_from_curve_and_encodings(td):
    f = td.Filmic.from_curve(CUDA, lambda x: x / (1.0 + x), desaturation=lambda x: 1.0 / (1.0 + x), encoding='gamma:2.0')
    n = spec.nodes()
    curve, G = tables(f)
    assert np.array_equal(curve[0], (n / (1 + n)).astype(F)) and np.array_equal(curve[1], (1 / (1 + n)).astype(F))
    assert np.array_equal(G, np.sqrt(spec.nodes(-16, 513)).astype(F)) and G[512] == 1.0
    srgb = td.Filmic(CUDA).host_encode.numpy()
    e = spec.nodes(-16, 513)
    assert srgb[512] == 1.0 and np.array_equal(srgb, np.where(e <= 0.0031308, 12.92 * e, 1.055 * e ** (1 / 2.4) - 0.055).astype(F))
    assert td.Filmic(CUDA, encoding=None).host_encode is None
    numpy_fn = td.Filmic.from_curve(CUDA, lambda x: np.tanh(x.numpy()))   # anything torch.as_tensor takes
    assert np.array_equal(numpy_fn.host_curve.numpy()[0], np.tanh(n).astype(F)) and (numpy_fn.host_curve.numpy()[1] == 1).all()
    for bad in ('rec709', 'gamma:', 'gamma:0', 'gamma:-1', 'gamma:x', 5):
        with pytest.raises(ValueError, match='encoding must be'):
            td.Filmic(CUDA, encoding=bad)
    with pytest.raises(ValueError, match='must give 1025 values'):
        td.Filmic.from_curve(CUDA, lambda x: x[:10])
    with pytest.raises(ValueError, match='must be finite'):
        td.Filmic.from_curve(CUDA, lambda x: x * 1e38)
    with pytest.raises(ValueError, match='desaturation must stay in 0..1'):
        td.Filmic.from_curve(CUDA, lambda x: x, desaturation=lambda x: x)
