"""CPU-only: the NumPy restatement of the colour transform (tests/colorlut_spec.py, the bits tests/test_gpu_colorlut.py holds the
kernel to) against independent evaluations -- a float64 computation of an affine LUT, the properties the header states (node hits,
neutral greys, tie order, clamping, the uint8 identity, the 1/255 constant) -- and the .cube parser of torch_darktable.ColorLUT."""

import numpy as np
import pytest

import colorlut_spec as spec

F = np.float32


def affine_lut(n, A, c):
    """(N, N, N, 3) float32 nodes of p -> A p + c sampled on [0, 1]^3, computed in float64 and rounded once; indexed [b, g, r]."""
    axis = np.arange(n, dtype=np.float64) / (n - 1)
    b, g, r = np.meshgrid(axis, axis, axis, indexing='ij')
    p = np.stack((r, g, b), axis=-1)
    return (p @ np.asarray(A, np.float64).T + np.asarray(c, np.float64)).astype(F)


def identity_lut(n):
    return affine_lut(n, np.eye(3), np.zeros(3))


def unit_scale(n):
    return (spec.scale_of(n, 0.0, 1.0),) * 3


A = np.array([[0.9, 0.15, -0.05], [0.02, 0.8, 0.18], [-0.1, 0.25, 0.85]])
C = np.array([0.01, -0.02, 0.03])


# ------------------------------------------------------------------ the 3D LUT
@pytest.mark.parametrize('n', [2, 5, 17, 33])
def test_affine_lut_is_reproduced_and_both_interpolations_agree(n):
    """Both interpolations are exact on an affine function; what remains is rounding: the float32 nodes (half an ulp each), the
    coordinate (a few ulp of a value up to N - 1, spread over a cell: |A| * N * 2^-23 / N) and four or seven float32 operations on
    values below 2.  A bound of 8 ulp of 2 covers that with room; an indexing or ordering mistake is off by a cell: >= 1 / 32."""
    rng = np.random.default_rng(n)
    x = rng.random((4000, 3)).astype(F)
    lut = affine_lut(n, A, C)
    want = x.astype(np.float64) @ A.T + C
    tol = 8 * 2.0 ** -22
    tet = spec.apply_lut(x, lut, (0, 0, 0), unit_scale(n), spec.TETRAHEDRAL)
    tri = spec.apply_lut(x, lut, (0, 0, 0), unit_scale(n), spec.TRILINEAR)
    assert tet.dtype == F and tri.dtype == F
    assert np.abs(tet - want).max() <= tol, np.abs(tet - want).max()
    assert np.abs(tri - want).max() <= tol, np.abs(tri - want).max()
    assert np.abs(tet.astype(np.float64) - tri).max() <= tol


def test_tetrahedral_differs_from_trilinear_on_a_curved_lut_and_matches_float64():
    """r * g * b is trilinear inside a cell, so trilinear interpolation reproduces it and tetrahedral does not: the two paths are
    really different.  Each is held to its own float64 evaluation written with explicit loops over the axes' order."""
    n = 3
    axis = np.arange(n, dtype=np.float64) / (n - 1)
    b, g, r = np.meshgrid(axis, axis, axis, indexing='ij')
    lut = np.stack((r * g * b, r * r, g + b * b), axis=-1).astype(F)
    rng = np.random.default_rng(7)
    x = rng.random((500, 3)).astype(F)
    tet = spec.apply_lut(x, lut, (0, 0, 0), unit_scale(n), spec.TETRAHEDRAL)
    tri = spec.apply_lut(x, lut, (0, 0, 0), unit_scale(n), spec.TRILINEAR)
    assert np.abs(tet - tri).max() > 1e-3
    L = lut.astype(np.float64)
    for i in range(len(x)):
        t = x[i].astype(np.float64) * (n - 1)
        k = np.minimum(t.astype(int), n - 2)
        f = t - k
        node = lambda p: L[p[2], p[1], p[0]]
        order = sorted(range(3), key=lambda c: -f[c])   # stable: ties keep r, g, b
        p = k.copy()
        acc = node(p).copy()
        for axis_ in order:
            q = p.copy()
            q[axis_] += 1
            acc += f[axis_] * (node(q) - node(p))
            p = q
        assert np.abs(tet[i] - acc).max() < 1e-6, i
        tri64 = sum(node(k + np.array([dr, dg, db])) * (f[0] if dr else 1 - f[0]) * (f[1] if dg else 1 - f[1]) * (f[2] if db else 1 - f[2])
                    for dr in (0, 1) for dg in (0, 1) for db in (0, 1))
        assert np.abs(tri[i] - tri64).max() < 1e-6, i


@pytest.mark.parametrize('interpolation', [spec.TETRAHEDRAL, spec.TRILINEAR])
@pytest.mark.parametrize('n', [2, 3, 17])
def test_a_coordinate_on_a_node_returns_the_nodes_bits(n, interpolation):
    """Domain [0, N - 1] makes the scale exactly 1: every integer coordinate is a node, the last one included (k = N - 2, f = 1)."""
    rng = np.random.default_rng(n)
    lut = rng.standard_normal((n, n, n, 3)).astype(F)
    idx = np.stack(np.meshgrid(*(np.arange(n),) * 3, indexing='ij'), axis=-1).reshape(-1, 3)   # (b, g, r)
    x = idx[:, ::-1].astype(F)
    scale = (spec.scale_of(n, 0.0, n - 1.0),) * 3
    assert scale[0] == F(1.0)
    out = spec.apply_lut(x, lut, (0, 0, 0), scale, interpolation)
    want = lut[idx[:, 0], idx[:, 1], idx[:, 2]]
    # f = 1 at the last node gives p + 1 * (q - p): q's bits when q - p is exact, within an ulp of q otherwise; nodes below the last have f = 0
    inner = (idx < n - 1).all(axis=1)
    assert np.array_equal(out[inner].view(np.int32), want[inner].view(np.int32))
    assert np.allclose(out, want, rtol=0, atol=4e-7)


def test_grey_stays_grey_under_tetrahedral_interpolation():
    """Diagonal nodes are grey (a tone curve), every other node is any colour.  With fr == fg == fb the walk is r, g, b and the two
    nodes off the diagonal cancel: f (L1 - L0) + f (L2 - L1) + f (L3 - L2) = f (L3 - L0).  In float32 they cancel up to the rounding
    of three steps on values below 4 (6 ulp of 4 bounds it); the trilinear result carries f (1 - f) of the coloured nodes."""
    n = 9
    rng = np.random.default_rng(3)
    tone = np.sort(rng.random(n)).astype(F)
    lut = rng.random((n, n, n, 3)).astype(F)
    lut[np.arange(n), np.arange(n), np.arange(n)] = tone[:, None]
    grey = np.repeat(rng.random((2000, 1)).astype(F), 3, axis=1)
    out = spec.apply_lut(grey, lut, (0, 0, 0), unit_scale(n), spec.TETRAHEDRAL)
    spread = out.max(axis=1) - out.min(axis=1)
    assert spread.max() <= 6 * 2.0 ** -21, spread.max()
    assert np.abs(out[:, 0] - np.interp(grey[:, 0].astype(np.float64), np.arange(n) / (n - 1), tone.astype(np.float64))).max() <= 6 * 2.0 ** -21
    tri = spec.apply_lut(grey, lut, (0, 0, 0), unit_scale(n), spec.TRILINEAR)
    assert (tri.max(axis=1) - tri.min(axis=1)).max() > 0.05
    # per-channel steps that are equal (the identity): grey to the bit
    out = spec.apply_lut(grey, identity_lut(n), (0, 0, 0), unit_scale(n), spec.TETRAHEDRAL)
    assert np.array_equal(out[:, 0].view(np.int32), out[:, 1].view(np.int32)) and np.array_equal(out[:, 1].view(np.int32), out[:, 2].view(np.int32))
    assert np.abs(out - grey).max() <= 2 ** -22


def test_ties_go_in_the_order_r_g_b():
    """With two fractions equal the two orders of the tied axes agree in exact arithmetic (the interpolation is continuous across
    the tetrahedra's faces) and differ in float32 rounding only: the tie rule decides bits.  A scalar float32 walk in the stated
    order must give the restatement's bits on every tied pixel, and the other order must give other bits on some of them."""
    rng = np.random.default_rng(4)
    lut = rng.random((2, 2, 2, 3)).astype(F)
    one = (F(1.0),) * 3

    def walk(f, order):
        p = [0, 0, 0]
        acc = lut[0, 0, 0].copy()
        for axis in order:
            q = list(p)
            q[axis] = 1
            acc = (acc + (F(f[axis]) * (lut[q[2], q[1], q[0]] - lut[p[2], p[1], p[0]]).astype(F)).astype(F)).astype(F)
            p = q
        return acc

    u, v = rng.random(300).astype(F), rng.random(300).astype(F)
    hi, lo = np.maximum(u, v), np.minimum(u, v)
    cases = {'fr == fg > fb': ((hi, hi, lo), (0, 1, 2), (1, 0, 2)), 'fb > fr == fg': ((lo, lo, hi), (2, 0, 1), (2, 1, 0)),
             'fg == fb > fr': ((lo, hi, hi), (1, 2, 0), (2, 1, 0)), 'fr > fg == fb': ((hi, lo, lo), (0, 1, 2), (0, 2, 1)),
             'fr == fb > fg': ((hi, lo, hi), (0, 2, 1), (2, 0, 1)), 'fg > fr == fb': ((lo, hi, lo), (1, 0, 2), (1, 2, 0)),
             'all equal': ((u, u, u), (0, 1, 2), (2, 1, 0))}
    for name, (f, order, other) in cases.items():
        x = np.stack(f, axis=-1)
        out = spec.apply_lut(x, lut, (0, 0, 0), one, spec.TETRAHEDRAL)
        stated = np.stack([walk(x[i], order) for i in range(len(x))])
        swapped = np.stack([walk(x[i], other) for i in range(len(x))])
        assert np.array_equal(out.view(np.int32), stated.view(np.int32)), name
        assert not np.array_equal(out.view(np.int32), swapped.view(np.int32)), name      # the rule is observable
        assert np.abs(out - swapped).max() < 1e-6, name                                   # ... in the last bits only


@pytest.mark.parametrize('interpolation', [spec.TETRAHEDRAL, spec.TRILINEAR])
def test_lut_clamps_outside_the_domain(interpolation):
    n = 4
    rng = np.random.default_rng(11)
    lut = rng.random((n, n, n, 3)).astype(F)
    lo, scale = (F(0.25),) * 3, (spec.scale_of(n, 0.25, 0.75),) * 3
    with np.errstate(invalid='ignore'):
        x = np.array([[-5.0, 0.5, 0.5], [0.25, 0.25, 0.25], [np.nan, np.nan, np.nan], [-np.inf, -np.inf, -np.inf], [0.0, -1.0, 0.1]], F)
    out = spec.apply_lut(x, lut, lo, scale, interpolation)
    assert np.isfinite(out).all()
    assert np.array_equal(out[1:4], np.repeat(lut[0, 0, 0][None], 3, axis=0))      # below the domain, NaN and -inf: the first node
    inside = spec.apply_lut(np.array([[0.25, 0.5, 0.5]], F), lut, lo, scale, interpolation)
    assert np.array_equal(out[0], inside[0])
    top = spec.apply_lut(np.array([[9.0, np.inf, 0.75]], F), lut, lo, scale, interpolation)
    assert np.allclose(top[0], lut[n - 1, n - 1, n - 1], rtol=0, atol=2e-7)


# ------------------------------------------------------------------ the shaper
@pytest.mark.parametrize('tables', [1, 3])
@pytest.mark.parametrize('s', [2, 5, 1024])
def test_shaper_against_float64_interpolation(s, tables):
    rng = np.random.default_rng(s + tables)
    table = np.sort(rng.random((tables, s)), axis=1).astype(F)
    lo, hi = -0.25, 1.5
    scale = spec.scale_of(s, lo, hi)
    x = (rng.random((3000, 3)) * 2.25 - 0.5).astype(F)
    x[0] = [np.nan, -np.inf, np.inf]
    x[1] = [lo, hi, 0.0]
    out = spec.apply_shaper(x, table[0] if tables == 1 else table, F(lo), scale)
    assert out.dtype == F
    grid = lo + (hi - lo) * np.arange(s) / (s - 1)
    for c in range(3):
        T = table[0 if tables == 1 else c].astype(np.float64)
        want = np.interp(np.nan_to_num(x[:, c].astype(np.float64), nan=lo, posinf=1e30, neginf=-1e30), grid, T)
        # rounding: the coordinate carries a few ulp of a value up to S - 1; the table's slope is at most 1 per cell
        assert np.abs(out[:, c] - want).max() <= 8 * 2.0 ** -23 * max(1.0, 1.0 * s / 64), (c, np.abs(out[:, c] - want).max())
    T0 = table[0]
    assert out[0, 0] == T0[0] and out[0, 1] == T0[0] if tables == 1 else out[0, 0] == table[0, 0] and out[0, 1] == table[1, 0]   # NaN, -inf: T[0]
    assert abs(out[0, 2] - table[-1 if tables == 3 else 0, -1]) <= 2e-7                                                         # +inf: T[S-1]
    assert out[1, 0] == table[0, 0]                                                                                             # x == lo: a node


# ------------------------------------------------------------------ matrix, load, store
def test_matrix_order_of_operations():
    m = np.array([[1.0, 2.0 ** -24, -1.0], [3.0, 5.0, 7.0], [0.0, 1.0, 0.0]], F)
    x = np.array([[1.0, 1.0, 1.0]], F)
    out = spec.apply_matrix(x, m)
    assert out[0, 0] == 0.0          # (1 + 2^-24) rounds to 1, then 1 - 1: the other order would leave 2^-24
    assert out[0, 1] == 15.0 and out[0, 2] == 1.0
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1000, 3)).astype(F)
    m = rng.standard_normal((3, 3)).astype(F)
    assert np.abs(spec.apply_matrix(x, m) - x.astype(np.float64) @ m.astype(np.float64).T).max() < 4e-6


def test_the_uint8_constant_and_the_identity_over_all_256_values():
    assert spec.C255.dtype == F and spec.C255.view(np.uint32) == 0x3B808081
    assert spec.C255 == F(1.0 / 255.0) and float(spec.C255) == float.fromhex('0x1.010102p-8')
    codes = np.arange(256, dtype=np.uint8)
    x = np.stack((codes, codes[::-1], codes), axis=-1)
    assert np.array_equal(spec.color_lut(x), x)
    v = spec.load(x)
    assert v.dtype == F and v.min() == 0.0 and np.abs(v[:, 0] - codes / 255.0).max() < 1e-7
    f = spec.color_lut(x, np.float32)
    assert np.array_equal(spec.color_lut(f, np.uint8), x)


def test_store_rounds_clamps_and_stores_zero_for_nan():
    with np.errstate(invalid='ignore'):
        v = np.array([[np.nan, -np.inf, np.inf], [-0.0, 1.5, 0.5], [0.5 / 255, 1.5 / 255, 2.5 / 255]], F)
    u = spec.store(v, np.uint8)
    assert u.tolist()[:2] == [[0, 0, 255], [0, 255, 128]]
    assert u[2].tolist() == np.rint(v[2] * F(255.0)).astype(int).tolist()
    h = spec.store(np.array([[1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0]], F), np.float16)
    assert h.dtype == np.float16 and h[0, 0] == 1.0 and h[0, 1] == np.float16(1.0 + 2.0 ** -9) and np.isinf(h[0, 2])   # ties to even
    x = np.random.default_rng(1).standard_normal((50, 3)).astype(np.float16)
    assert np.array_equal(spec.color_lut(x).view(np.int16), x.view(np.int16))
    x32 = np.random.default_rng(2).standard_normal((50, 3)).astype(F)
    x32[0, 0] = -0.0
    assert np.array_equal(spec.color_lut(x32).view(np.int32), x32.view(np.int32))


def test_stages_run_in_the_order_matrix_shaper_lut():
    rng = np.random.default_rng(9)
    x = rng.random((200, 3)).astype(F)
    m = (np.eye(3) * 0.5 + 0.1).astype(F)
    table = (np.linspace(0, 1, 33) ** 2).astype(F)
    lut = affine_lut(5, A, C)
    scale, ls = spec.scale_of(33, 0, 1), unit_scale(5)
    all_three = spec.color_lut(x, None, m, table, F(0), scale, lut, (0, 0, 0), ls)
    by_hand = spec.apply_lut(spec.apply_shaper(spec.apply_matrix(x, m), table, F(0), scale), lut, (0, 0, 0), ls)
    assert np.array_equal(all_three, by_hand)
    assert not np.array_equal(all_three, spec.apply_matrix(spec.apply_lut(spec.apply_shaper(x, table, F(0), scale), lut, (0, 0, 0), ls), m))


# ------------------------------------------------------------------ the .cube parser
CUBE_3D = """# a comment
TITLE "test look"

LUT_3D_SIZE 2
DOMAIN_MIN 0.0 0.0 0.0
DOMAIN_MAX 1.0 2.0 4.0
0 0 0
1 0 0
0 1 0
1 1 0
  # a comment between rows
0 0 1
1 0 1
0 1 1
1 1 1.5
"""

CUBE_1D = """TITLE "curve"
LUT_1D_SIZE 3
0.0 0.1 0.2
0.5 0.6 0.7
1.0 1.1 1.2
"""


def test_cube_parser_reads_3d_1d_domains_and_comments(td, tmp_path):
    import torch
    from torch_darktable.colorlut import parse_cube

    dev = torch.device('cuda', 0)   # a device object only: the tables reach a GPU only where there is one
    kind, size, lo, hi, rows = parse_cube(CUBE_3D)
    assert (kind, size, lo, hi) == ('3D', 2, (0.0, 0.0, 0.0), (1.0, 2.0, 4.0)) and len(rows) == 8 and rows[-1] == [1.0, 1.0, 1.5]
    c = td.ColorLUT.from_cube(CUBE_3D, dev)
    assert c.lut_size == 2 and c.shaper is None and c.matrix is None and c.interpolation == 'tetrahedral'
    assert c.lut[1, 1, 1].tolist() == [1.0, 1.0, 1.5] and c.lut[0, 0, 1].tolist() == [1.0, 0.0, 0.0] and c.lut[1, 0, 0].tolist() == [0.0, 0.0, 1.0]   # [b, g, r]
    assert c.lut_lo == (0.0, 0.0, 0.0) and c.lut_scale == (1.0, 0.5, 0.25)
    path = tmp_path / 'look.cube'
    path.write_text(CUBE_3D)
    for source in (path, str(path)):
        again = td.ColorLUT.from_cube(source, dev, interpolation='trilinear')
        assert torch.equal(again.lut, c.lut) and again.lut_scale == c.lut_scale and again.interpolation == 'trilinear'
    s = td.ColorLUT.from_cube(CUBE_1D, dev, matrix=np.eye(3))
    assert s.lut is None and s.shaper_size == 3 and s.shaper_tables == 3 and s.matrix == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    assert s.shaper.tolist() == [[0.0, 0.5, 1.0], [F(0.1), F(0.6), F(1.1)], [F(0.2), F(0.7), F(1.2)]]
    assert s.shaper_lo == 0.0 and s.shaper_scale == 2.0
    ranged = td.ColorLUT.from_cube(CUBE_1D.replace('LUT_1D_SIZE 3', 'LUT_1D_SIZE 3\nDOMAIN_MIN -1 -1 -1\nDOMAIN_MAX 3 3 3'), dev)
    assert ranged.shaper_lo == -1.0 and ranged.shaper_scale == 0.5
    resolve = td.ColorLUT.from_cube(CUBE_1D.replace('LUT_1D_SIZE 3', 'LUT_1D_SIZE 3\nLUT_1D_INPUT_RANGE 0.0 4.0'), dev)
    assert resolve.shaper_scale == 0.5
    # a parsed identity reproduces identity()
    n = 3
    text = f'LUT_3D_SIZE {n}\n' + ''.join(f'{r / (n - 1)!r} {g / (n - 1)!r} {b / (n - 1)!r}\n' for b in range(n) for g in range(n) for r in range(n))
    assert torch.equal(td.ColorLUT.from_cube(text, dev).lut, td.ColorLUT.identity(dev, n).lut)
    assert np.array_equal(td.ColorLUT.identity(dev, 5).lut.numpy(), identity_lut(5))


@pytest.mark.parametrize('text, line, what', [
    (CUBE_3D.replace('DOMAIN_MIN', 'LUT_1D_SIZE 4\nDOMAIN_MIN'), 5, 'second size'),
    (CUBE_3D.replace('1 1 1.5\n', ''), 14, '7 rows'),
    (CUBE_3D + '0 0 0\n', 16, 'more rows'),
    (CUBE_3D.replace('LUT_3D_SIZE 2', 'LUT_3D_SIZE 1'), 4, 'size must be 2..65'),
    (CUBE_3D.replace('LUT_3D_SIZE 2', 'LUT_3D_SIZE 66'), 4, 'size must be 2..65'),
    (CUBE_1D.replace('LUT_1D_SIZE 3', 'LUT_1D_SIZE 1025'), 2, 'size must be 2..1024'),
    (CUBE_3D.replace('LUT_3D_SIZE 2', 'LUT_3D_SIZE two'), 4, 'one integer'),
    (CUBE_3D.replace('1 0 1\n', '1 nan 1\n'), 13, 'non-finite'),
    (CUBE_3D.replace('1 0 1\n', '1 inf 1\n'), 13, 'non-finite'),
    (CUBE_3D.replace('1 0 1\n', '1 0\n'), 13, 'three numbers'),
    (CUBE_3D.replace('1 0 1\n', '1 0 1 1\n'), 13, 'three numbers'),
    (CUBE_3D.replace('1 0 1\n', '1 zero 1\n'), 13, 'not a keyword'),
    (CUBE_3D.replace('DOMAIN_MAX 1.0 2.0 4.0', 'DOMAIN_MAX 1.0 2.0'), 6, '3 finite numbers'),
    (CUBE_3D.replace('DOMAIN_MAX 1.0 2.0 4.0', 'DOMAIN_MAX 1.0 inf 4.0'), 6, '3 finite numbers'),
    ('0 0 0\n' + CUBE_3D, 1, 'in front of'),
    ('# nothing\nTITLE "x"\n', 2, 'without LUT_3D_SIZE'),
], ids=['both-sizes', 'row-missing', 'row-too-many', 'size-1', 'size-66', 'size-1d-1025', 'size-word', 'nan', 'inf', 'two-numbers', 'four-numbers', 'word-in-row',
        'domain-two-values', 'domain-inf', 'row-before-size', 'no-size'])
def test_cube_parser_rejects_malformed_text_naming_the_line(td, text, line, what):
    import torch

    with pytest.raises(ValueError, match=f'line {line}\\b') as e:
        td.ColorLUT.from_cube(text, torch.device('cuda', 0))
    assert what in str(e.value), str(e.value)


def test_cube_1d_file_with_per_channel_domain_is_refused(td):
    import torch

    with pytest.raises(ValueError, match='same domain'):
        td.ColorLUT.from_cube(CUBE_1D.replace('LUT_1D_SIZE 3', 'LUT_1D_SIZE 3\nDOMAIN_MAX 1 2 1'), torch.device('cuda', 0))
    with pytest.raises(ValueError, match='distinct ends'):
        td.ColorLUT.from_cube(CUBE_3D.replace('DOMAIN_MAX 1.0 2.0 4.0', 'DOMAIN_MAX 1.0 0.0 4.0'), torch.device('cuda', 0))
