"""GPU: the colour and tone-map kernels (csrc/color.hip, csrc/tonemap.hip, csrc/tdk_color.h) over their whole input domain.

tests/test_gpu_parity.py holds these kernels to the oracle on one well-exposed scene with a flat tolerance.  Here they run on the
pixel sets of tests/color_domain_spec.py -- in gamut, [-0.25, 1.6], dense around 0, greys, a few ulps on either side of every
branch constant, Lab with L outside [0, 1] -- and on special values (0, -0, 1, the metrics' means, -1, 65504, FLT_MAX, +-inf,
NaN), and are held to the NaN-faithful float64 specification of that module:
  float outputs   |gpu - spec| <= 8 * (A_op + K_op * s_i) * scale on every non-excluded value (8x the bound the fp32 C oracle meets,
                  tests/test_color_domain_spec.py: v_log_f32, v_exp_f32 and v_rcp_f32 are ~1 ulp each and exp2(y * log2 x)
                  multiplies the log's error by |y * log2 x|, where libm's powf stays near 1 ulp); for float16 storage the
                  specification sees the rounded input and the result may be rounded once more (half a binary16 ulp);
                  NaN positions are the specification's;
  uint8 outputs   floor(clip(spec) * 255 + 0.5), one step off only where spec * 255 lies within 255x the value's bound of a
                  rounding tie; per tone mapper, no more such values than four times what the oracle shows on the same pixels;
  excluded        at most 1 % of a case (a bound above 1e-3: ill-conditioned in the reference itself).
Paths: N = 4 k pixels run the vector body, 4 k + 1 and 4 k + 3 body and tail, a view that starts one pixel into an allocation
the tail kernel alone.  Tone mappers: vibrance 0 with a finite gamma runs the LEAN instantiation, everything else the full one.
Special pixels: the tone mappers and the clipping operators give the oracle's output where a NaN, an overflow or the clip
decides it, and every other value is held to the specification or to the oracle's value; the conversions have the oracle's NaN
positions and infinities."""

import numpy as np
import pytest
import torch

import color_domain_spec as S

pytestmark = pytest.mark.gpu

PATHS = ['body', 'body_tail1', 'body_tail3', 'tail_view']
DTYPES = {'f32': torch.float32, 'f16': torch.float16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def f16_ulp(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.where(np.isfinite(v), v, 1.0)), 2.0 ** -14))) - 10)


def place(a, path, dev, dtype):
    """(1, n, C) device tensor of the first n rows of `a` for `path`; the view starts one pixel into its allocation."""
    n = a.shape[0] - {'body': a.shape[0] % 4, 'body_tail1': a.shape[0] % 4 - 1}.get(path, 0)
    t = torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev).to(dtype)
    if path != 'tail_view':
        assert t.data_ptr() % 16 == 0
        return t[None], n
    pool = torch.zeros((1, n + 1) + tuple(t.shape[1:]), dtype=dtype, device=dev)
    v = pool[:, 1:]
    v.copy_(t[None])
    assert v.is_contiguous() and v.data_ptr() % (4 * t.element_size()) != 0
    return v, n


def run_case(td, dev, case, x, path, dtype):
    """The kernel of `case` on input x (N, C) float32: (result as float64 (n, M), n, result dtype)."""
    key, op, kind, params = case
    t, n = place(x[:, :3], path, dev, DTYPES[dtype])
    if op.startswith('tonemap_'):
        m = torch.tensor(params[0], dtype=torch.float32, device=dev)
        p = td.TonemapParameters(*params[1:])
        mode = op[len('tonemap_'):]
        out = (td.reinhard_tonemap(t, m, p) if mode == 'reinhard' else td.linear_tonemap(t, m, p) if mode == 'linear'
               else td.aces_tonemap(t, p) if mode == 'aces' else td.aces_tonemap(t, p, m))
        assert out.dtype == torch.uint8 and out.shape == t.shape
    elif op == 'compute_luminance':
        out = td.compute_luminance(t)[..., None]
    elif op == 'compute_log_luminance':
        out = td.compute_log_luminance(t, S.LOG_EPS)[..., None]
    elif op in ('modify_luminance', 'modify_log_luminance'):
        lum, _ = place(x[:, 3], path, dev, torch.float32)
        out = td.modify_luminance(t, lum) if op == 'modify_luminance' else td.modify_log_luminance(t, lum, S.LOG_EPS)
    elif op == 'normalize_image':
        from torch_darktable.pipeline.util import normalize_image
        out = normalize_image(t, torch.tensor(params, dtype=torch.float32, device=dev))
    else:
        out = getattr(td, op)(t, *(params or ()))
    return out[0].detach().cpu().to(torch.float64).numpy(), n, out.dtype


def gpu_bounds(case, dtype, special=False):
    x, r, s, sc, pre = S.case_spec(case, dtype, special)
    return x, r, S.bound(case[0], s, sc, pre, S.GPU_FACTOR), S.excluded(case[0], s, sc, pre)


def describe(x, got, r, bad):
    i = np.argwhere(bad)[0][0]
    return f'{bad.sum()} values; first at pixel {i}: input {x[i]}, kernel {got[i]}, specification {r[i]}'


# ------------------------------------------------------------------ colour operators, luminance extract / replace, normalize_image
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('case', S.COLOR_CASES, ids=S.case_id)
def test_color_kernels_whole_domain(td, dev, case, path, dtype):
    x, r, b, ex = gpu_bounds(case, dtype)
    got, n, out_dtype = run_case(td, dev, case, x, path, dtype)
    x, r, b, ex = x[:n], r[:n], b[:n], ex[:n]
    assert ex.mean() <= S.EXCLUDE_CAP, ex.mean()
    assert np.array_equal(np.isnan(got), np.isnan(r)), 'NaN positions: ' + describe(x, got, r, np.isnan(got) != np.isnan(r))
    if out_dtype == torch.float16:
        b = b + 0.5 * f16_ulp(np.maximum(np.abs(got), np.abs(r)))
    bad = ~ex & ~(S._absdiff(got, r) <= b)
    assert not bad.any(), describe(x, got, r, bad)


# ------------------------------------------------------------------ tone mappers
def check_u8(x, got, r, b, ex):
    q = S.quantise(r)
    dq = np.abs(got - q)
    assert (dq[~ex] <= 1).all(), describe(x, got, q, ~ex & (dq > 1))
    off = ~ex & (dq > 0) & ~(S.tie_distance(r) <= 255.0 * b)
    assert not off.any(), 'one uint8 step off, and not on a rounding tie: ' + describe(x, got, r * 255.0, off)
    return int((dq > 0).sum())


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('case', S.TONEMAP_CASES, ids=S.case_id)
def test_tonemap_kernels_whole_domain(td, dev, case, path, dtype):
    x, r, b, ex = gpu_bounds(case, dtype)
    got, n, _ = run_case(td, dev, case, x, path, dtype)
    assert ex[:n].mean() <= S.EXCLUDE_CAP, ex[:n].mean()
    off = check_u8(x[:n], got, r[:n], b[:n], ex[:n])
    # the oracle is one step off on 0 to 3 of a case's 59 997 values (CONSTANTS records the operator's largest count): a share of
    # that size says nothing case by case, so each case, path and storage type is held to 4x the operator's recorded count here
    # and test_tonemap_tie_share holds the operator to 4x the oracle's count on the same pixels
    assert off <= 4 * S.CONSTANTS[case[0]][3], off


@pytest.mark.parametrize('mode', S.TONEMAP_MODES)
def test_tonemap_tie_share(td, oracle, dev, mode):
    """Over the operator's parameter sets: the kernel is one uint8 step away from the specification on no more values than four
    times what the fp32 oracle shows on the same pixels (the constants are per operator, and so is this share: single cases
    hold two or three such values out of 60 000), for both storage types, on the vector body and on the tail kernel."""
    for dtype in ('f32', 'f16'):
        for path in ('body_tail3', 'tail_view'):
            n_gpu = n_oracle = 0
            for case in S.TONEMAP_CASES:
                if case[0] != 'tonemap_' + mode:
                    continue
                x, r, b, ex = gpu_bounds(case, dtype)
                got, n, _ = run_case(td, dev, case, x, path, dtype)
                n_gpu += check_u8(x, got, r, b, ex)
                n_oracle += int((S.oracle_run(oracle, case, x)[1].astype(np.float64) != S.quantise(r)).sum())
            print(f'{mode} {dtype} {path}: kernel {n_gpu}, oracle {n_oracle} of {9 * 3 * S.N_PIXELS} values one step off')
            assert n_gpu <= 4 * n_oracle, (dtype, path, n_gpu, n_oracle)


# ------------------------------------------------------------------ special pixels
SPECIAL_PATHS = ['body', 'body_tail3', 'tail_view']


@pytest.mark.parametrize('path', SPECIAL_PATHS)
@pytest.mark.parametrize('case', S.TONEMAP_CASES, ids=S.case_id)
def test_tonemap_special_pixels(td, oracle, dev, case, path):
    """Every value of the special frame is checked (color_domain_spec.special_classes; the class sizes are pinned by
    tests/test_color_domain_spec.py): the oracle's uint8 where the oracle decides it; floor(clip(spec) * 255 + 0.5), one step off
    only on a rounding tie, on the other well-conditioned values; within the bound of the oracle's value on the ill-conditioned
    ones (next to a 65504 channel the Lab round trip runs at 1e10, where the reference's two 3x3 matrices, inverse to seven
    digits only, move the other channels by thousands)."""
    x, r, b, ou8, exact, tied, loose = S.special_classes(oracle, case)
    got, n, _ = run_case(td, dev, case, x, path, 'f32')
    x, r, b, ou8, exact, tied, loose = x[:n], r[:n], b[:n], ou8[:n], exact[:n], tied[:n], loose[:n]
    bad = exact & (got != ou8)
    assert not bad.any(), describe(x, got, ou8, bad)
    check_u8(x, got, r, b, ~tied)
    with np.errstate(all='ignore'):
        bad = loose & ~(np.abs(got - ou8) <= 255.0 * b + 1.0)
    assert not bad.any(), describe(x, got, ou8, bad)


@pytest.mark.parametrize('path', SPECIAL_PATHS)
@pytest.mark.parametrize('case', S.COLOR_CASES, ids=S.case_id)
def test_color_special_pixels(td, oracle, dev, case, path):
    """The oracle's NaN positions and infinities on every value.  The clipping operators (modify_*): the oracle's value wherever
    the oracle decides it (a NaN, an overflow, the clip), inside the specification's bound on the other well-conditioned values,
    within the bound of the oracle's value on the ill-conditioned ones -- the 65504, FLT_MAX and infinite rows included.  The
    conversions: every finite value inside the specification's bound (whatever its size) and within that bound of the oracle's."""
    x, r, b, of, exact, tied, loose = S.special_classes(oracle, case)
    got, n, _ = run_case(td, dev, case, x, path, 'f32')
    x, r, b, of, exact, tied, loose = x[:n], r[:n], b[:n], of[:n], exact[:n], tied[:n], loose[:n]
    assert np.array_equal(np.isnan(got), np.isnan(of)), 'NaN positions: ' + describe(x, got, of, np.isnan(got) != np.isnan(of))
    inf = np.isinf(of) | np.isinf(got)
    assert np.array_equal(got[inf], of[inf]), describe(x, got, of, inf & (got != of))
    fin = np.isfinite(of) & np.isfinite(got)
    with np.errstate(all='ignore'):
        near_oracle = S._absdiff(got, of) <= 1.125 * b   # the oracle itself lies within an eighth of the bound of the specification
        near_spec = S._absdiff(got, r) <= b
    if case[1].startswith('modify_'):
        bad = exact & (got != of)
        assert not bad.any(), describe(x, got, of, bad)
        bad = fin & tied & ~near_spec
        assert not bad.any(), describe(x, got, r, bad)
        bad = fin & loose & ~near_oracle
        assert not bad.any(), describe(x, got, of, bad)
    else:
        bad = fin & ~(near_spec & near_oracle)
        assert not bad.any(), describe(x, got, of, bad)
