"""GPU: antialiased scaling (torch_darktable.Resize, include/tdk_hip_resample.h) against the float64 restatement of its
specification, `resize_ref` of tests/test_resample_spec.py (pinned there to torch's CPU antialiased interpolate).

Tolerances.  u = 2^-24 is the unit round-off of float32, n_x and n_y the largest tap counts of the two axes, X = max|x|.

  float32   |y - y64| <= (2 (n_x + n_y) + 12) u X.  Derivation, per pass with n taps on values bounded by X: the weights are
            non-negative and sum to 1, so every partial sum is bounded by X (1 + O(u)).  Accumulating n products rounds n times,
            each by at most u X: n u X.  The weights themselves are rounded: each normalised weight carries a few relative
            roundings (forming it, the sum, the division), and since sum_j w_j |x_j| <= X a relative error of k u in every
            weight moves the result by at most k u X; with the sum of n rounded weights drifting by up to n u / 2 from 1 this is
            covered by another n u X.  Converting the stored value to float32 (exact for all three types), the final division or
            scaling and the store add a few u X: 6 u X per pass.  The vertical pass works on the horizontal results, which are
            bounded by X (1 + (2 n_x + 6) u), and passes the horizontal error on with weights that sum to 1, so the two passes add:
            (2 n_x + 6) + (2 n_y + 6) = 2 (n_x + n_y) + 12.  Terms of order u^2 are below 1e-5 of the bound at n <= 33.
  binary16  the float32 bound plus half a binary16 ulp of the exact value (one rounding to nearest even at the store); the
            reference runs on the binary16-rounded input.
  uint8     equal to rint(y64); +-1 is excused only where y64 lies within the float32 bound (X = 255, in LSB) of a k + 1/2 tie,
            and at most 1 % of a case's values may be excused.

Every parity check prints its figures (pytest -s) before it asserts."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('resample_spec', Path(__file__).resolve().parent / 'test_resample_spec.py')
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)
resize_ref, max_taps, checkerboard = spec.resize_ref, spec.max_taps, spec.checkerboard

U = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements past an aligned allocation (a slice of a larger
    buffer), so that its address is not a multiple of 16 bytes."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


def run(td, dev, x, dst, offset=0):
    """x: (H, W, C) NumPy array; dst = (oh, ow)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if offset:
        t = at_offset(t, offset)
    out = td.Resize(dev, (x.shape[1], x.shape[0]), (dst[1], dst[0])).process(t)
    assert tuple(out.shape) == (dst[0], dst[1], x.shape[2]) and out.dtype == t.dtype and out.is_contiguous()
    return out.cpu().numpy()


def bound_f32(src, dst, xmax):
    n_x, n_y = max_taps(src[1], dst[1]), max_taps(src[0], dst[0])
    return (2 * (n_x + n_y) + 12) * U * xmax, (n_x, n_y)


def half_ulp_f16(v):
    """Half a binary16 ulp of |v| (subnormals: 2^-25)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 11)


def check_f32(td, dev, x, dst, what='', offset=0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y64 = resize_ref(x, dst[1], dst[0])
    tol, taps = bound_f32(x.shape, dst, float(np.abs(x).max()))
    err = float(np.abs(run(td, dev, x, dst, offset).astype(np.float64) - y64).max())
    print(f'resize f32 {what}{x.shape} -> {dst} taps {taps}: err {err:.3e} bound {tol:.3e} ({err / tol if tol else 0:.2f} of it)')
    assert err <= tol, (x.shape, dst, err, tol)
    return y64


def check_f16(td, dev, x, dst, what='', offset=0):
    x16 = np.ascontiguousarray(x).astype(np.float16)
    y64 = resize_ref(x16, dst[1], dst[0])
    tol, taps = bound_f32(x16.shape, dst, float(np.abs(x16.astype(np.float64)).max()))
    got = run(td, dev, x16, dst, offset)
    assert got.dtype == np.float16
    over = np.abs(got.astype(np.float64) - y64) - (tol + half_ulp_f16(y64))
    print(f'resize f16 {what}{x16.shape} -> {dst} taps {taps}: worst excess over (f32 bound + half ulp) {float(over.max()):.3e}, '
          f'{float((got != y64.astype(np.float16)).mean()):.2e} of the values differ from the rounded reference')
    assert (over <= 0).all(), (x16.shape, dst, float(over.max()))


def check_u8(td, dev, x, dst, what='', offset=0):
    assert x.dtype == np.uint8
    y64 = resize_ref(x, dst[1], dst[0])
    tol, taps = bound_f32(x.shape, dst, 255.0)
    got = run(td, dev, x, dst, offset).astype(np.int64)
    want = np.rint(y64).astype(np.int64)
    diff = got - want
    near_tie = np.abs(y64 - (np.floor(y64) + 0.5)) <= tol
    # where the exact value sits within the bound of a tie, either neighbour of the tie is a correct rounding
    other = np.where(near_tie, np.floor(y64).astype(np.int64) + (want == np.floor(y64)), want)
    excused = (diff != 0) & near_tie & (got == other)
    wrong = (diff != 0) & ~excused
    print(f'resize u8 {what}{x.shape} -> {dst} taps {taps}: {int((diff != 0).sum())} of {diff.size} differ from rint(y64), '
          f'{int(excused.sum())} excused by a tie within {tol:.2e} LSB ({float(near_tie.mean()):.2e} of the values are that close), {int(wrong.sum())} wrong')
    assert not wrong.any(), (x.shape, dst, int(wrong.sum()), int(np.abs(diff).max()))
    assert excused.mean() <= 0.01, (x.shape, dst, float(excused.mean()))


def rand_f(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# (h, w) -> (oh, ow): the issue's six, then ratio exactly 16, a different ratio per axis (down / up mixed), odd sizes, near-identity
GEOMETRIES = [
    ((768, 1024), (192, 256)), ((768, 1024), (48, 64)), ((750, 1000), (187, 250)), ((301, 403), (75, 100)), ((250, 334), (17, 23)),
    ((97, 131), (200, 301)),
    ((256, 512), (16, 32)), ((160, 1600), (40, 100)), ((96, 50), (12, 175)), ((37, 53), (80, 91)), ((101, 77), (100, 76)), ((129, 257), (9, 17)),
]


# ------------------------------------------------------------------ 1. parity on random images
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('src,dst', GEOMETRIES)
def test_parity_f32(td, dev, src, dst, c):
    check_f32(td, dev, rand_f((*src, c), src[0] + dst[1] + c), dst)


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('src,dst', GEOMETRIES)
def test_parity_f16(td, dev, src, dst, c):
    check_f16(td, dev, rand_f((*src, c), src[1] + dst[0] + c), dst)


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('src,dst', GEOMETRIES + [((64, 96), (64, 96))])
def test_parity_u8(td, dev, src, dst, c):
    check_u8(td, dev, rand_u8((*src, c), src[0] * 3 + dst[1] + c), dst)


def test_signed_and_large_values_f32(td, dev):
    """The bound scales with max|x|: values in [-1000, 1000)."""
    check_f32(td, dev, (rand_f((301, 403, 3), 9) - 0.5) * 2000.0, (75, 100), 'signed ')


# ------------------------------------------------------------------ 2. identity, degenerate shapes
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('size', [(64, 96), (1, 1), (37, 53), (200, 301)])
def test_identity_size_returns_the_bits(td, dev, size, c):
    f = (rand_f((*size, c), 3) - 0.5) * 8.0
    f.flat[0] = -0.0
    assert np.array_equal(run(td, dev, f, size).view(np.uint32), f.view(np.uint32))
    h = f.astype(np.float16)
    assert np.array_equal(run(td, dev, h, size).view(np.uint16), h.view(np.uint16))
    u = rand_u8((*size, c), 4)
    assert np.array_equal(run(td, dev, u, size), u)


@pytest.mark.parametrize('c', [1, 3])
def test_one_by_one_output_single_rows_and_single_columns(td, dev, c):
    for src, dst in (((16, 16), (1, 1)), ((5, 7), (1, 1)), ((1, 1), (1, 1)), ((1, 1), (5, 9)), ((1, 640), (1, 40)), ((1, 100), (1, 333)),
                     ((640, 1), (40, 1)), ((77, 1), (200, 1)), ((1, 50), (3, 20)), ((50, 1), (20, 3)), ((3, 1000), (1, 250))):
        check_f32(td, dev, rand_f((*src, c), 11), dst, 'thin ')
        check_f16(td, dev, rand_f((*src, c), 12), dst, 'thin ')
        check_u8(td, dev, rand_u8((*src, c), 13), dst, 'thin ')


def test_ratio_exactly_16_on_both_axes(td, dev):
    for src, dst in (((1024, 2048), (64, 128)), ((16, 16), (1, 1)), ((1600, 48), (100, 3))):
        check_f32(td, dev, rand_f((*src, 3), 21), dst, '16:1 ')
        check_u8(td, dev, rand_u8((*src, 3), 22), dst, '16:1 ')
    with pytest.raises(ValueError, match='ratio'):
        td.Resize(dev, (2049, 1024), (128, 64))


def test_a_60000_wide_row_keeps_its_positions(td, dev):
    """1 x 60 000 -> 1 x 4 000 (15:1, 30 taps): s (i + 1/2) formed in float32 would be off by up to 4e-3 of a pixel at the far
    end, which moves every weight by about 4e-3 / 15 and a result on white noise by about 1e-4, against a bound of 4e-6.
    Sizes up to 65535, a tall column as well."""
    src, dst = (1, 60000), (1, 4000)
    check_f32(td, dev, rand_f((*src, 1), 31), dst, 'wide noise ')
    check_f32(td, dev, rand_f((*src, 3), 32), dst, 'wide noise ')
    ramp = np.arange(60000, dtype=np.float32).reshape(1, 60000, 1) / 60000.0
    y = check_f32(td, dev, ramp, dst, 'wide ramp ')
    assert abs(y[0, -2, 0] - (3998.5 * 15.0 - 0.5) / 60000.0) < 1e-7   # an interior output of a ramp is the ramp at its centre (sample j sits at j + 1/2)
    check_u8(td, dev, rand_u8((2, 65535, 1), 33), (1, 4096), 'widest ')
    check_f32(td, dev, rand_f((40001, 1, 1), 34), (2501, 1), 'tall ')


# ------------------------------------------------------------------ 3. alignment
@pytest.mark.parametrize('c', [1, 3])
def test_unaligned_offset_views(td, dev, c):
    """Source views one and three elements past an aligned buffer (4, 2 or 1 bytes per element): the same results as aligned."""
    for src, dst in (((301, 403), (75, 100)), ((97, 131), (200, 301)), ((250, 334), (17, 23))):
        for off in (1, 3):
            f, u = rand_f((*src, c), 41), rand_u8((*src, c), 42)
            check_f32(td, dev, f, dst, f'offset {off} ', off)
            check_f16(td, dev, f, dst, f'offset {off} ', off)
            check_u8(td, dev, u, dst, f'offset {off} ', off)
            assert np.array_equal(run(td, dev, u, dst, off), run(td, dev, u, dst))
            assert np.array_equal(run(td, dev, f, dst, off), run(td, dev, f, dst))


def test_output_into_an_unaligned_destination(td, dev):
    """The C entry point with a destination one element past an aligned buffer."""
    from torch_darktable._native import lib
    u = rand_u8((250, 334, 3), 43)
    t = torch.from_numpy(u).to(dev)
    pool = torch.zeros(17 * 23 * 3 + 32, dtype=torch.uint8, device=dev)
    out = pool[1:1 + 17 * 23 * 3]
    assert out.data_ptr() % 2 == 1
    rc = lib.tdk_resample(t.data_ptr(), out.data_ptr(), 334, 250, 23, 17, 3, 2, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tdk_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.view(17, 23, 3).cpu().numpy(), run(td, dev, u, (17, 23)))
    assert int(pool[0]) == 0 and int(pool[1 + 17 * 23 * 3:].max()) == 0   # nothing written outside the destination


# ------------------------------------------------------------------ 4. full frames
@pytest.mark.parametrize('dst', [(768, 1024), (192, 256)])
def test_12mp_frame_u8_and_f16(td, dev, dst):
    src = (3072, 4096)
    check_u8(td, dev, rand_u8((*src, 3), 51), dst, '12 MP ')
    check_f16(td, dev, rand_f((*src, 3), 52), dst, '12 MP ')


# ------------------------------------------------------------------ 5. what the filter is for
def test_constant_image_stays_constant(td, dev):
    for src, dst in (((301, 403), (75, 100)), ((250, 334), (17, 23)), ((97, 131), (200, 301)), ((256, 512), (16, 32))):
        for value in (0.7, 1.0, 123.456):
            x = np.full((*src, 3), value, np.float32)
            tol, _ = bound_f32(src, dst, value)
            got = run(td, dev, x, dst).astype(np.float64)
            print(f'constant {value} {src} -> {dst}: off by at most {float(np.abs(got - np.float64(np.float32(value))).max()):.3e}, bound {tol:.3e}')
            assert np.abs(got - np.float64(np.float32(value))).max() <= tol
        for value in (0, 1, 77, 255):
            assert (run(td, dev, np.full((*src, 3), value, np.uint8), dst) == value).all()


def test_checkerboard_at_4_to_1_comes_out_flat(td, dev):
    """2 x 2-pixel squares placed so that plain bilinear at 4:1 reads a single colour (pipeline.util.resize returns 0 everywhere,
    although half the pixels are 1); the antialiased filter returns the mean away from the frame's edge."""
    from torch_darktable.pipeline.util import resize
    x = checkerboard(256, 384).astype(np.float32)
    plain = resize(torch.from_numpy(x).to(dev), (64, 96)).cpu().numpy()
    assert np.abs(plain).max() == 0.0
    tol, _ = bound_f32((256, 384), (64, 96), 1.0)
    got = run(td, dev, x, (64, 96))
    assert np.abs(got[1:-1, 1:-1].astype(np.float64) - 0.5).max() <= tol
    check_f32(td, dev, x, (64, 96), 'checkerboard ')
    u = (x * 255).astype(np.uint8)
    got8 = run(td, dev, u, (64, 96))
    assert set(np.unique(got8[1:-1, 1:-1])) <= {127, 128}   # 127.5 is a tie: either neighbour
    check_u8(td, dev, np.repeat(u, 3, axis=2), (64, 96), 'checkerboard ')


# ------------------------------------------------------------------ 6. front-end errors that need a device, determinism, graph
def test_non_contiguous_and_wrong_type_inputs(td, dev):
    rs = td.Resize(dev, (64, 48), (16, 12))
    with pytest.raises(RuntimeError, match='contiguous'):
        rs.process(torch.zeros(48, 128, 3, device=dev)[:, ::2])
    with pytest.raises(RuntimeError, match='contiguous'):
        rs.process(torch.zeros(3, 48, 64, device=dev).permute(1, 2, 0))
    with pytest.raises(RuntimeError, match='float32, float16 or uint8'):
        rs.process(torch.zeros(48, 64, 3, device=dev, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='CUDA'):
        rs.process(torch.zeros(48, 64, 3))


def test_two_runs_are_bit_identical(td, dev):
    for dtype, dst in ((torch.float32, (187, 250)), (torch.float16, (48, 64)), (torch.uint8, (187, 250))):
        x = torch.from_numpy(rand_f((750, 1000, 3), 61) * 255).to(dev).to(dtype)
        rs = td.Resize(dev, (1000, 750), (dst[1], dst[0]))
        a, b = rs.process(x), rs.process(x)
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.uint8])
def test_graph_capture_from_the_first_call(td, dev, dtype):
    """A geometry no earlier call of this process has used, captured on one stream without a warm-up call; the replay equals the
    eager result bit for bit, also after the input buffer's contents change."""
    src, dst = (431, 577), (108, 145)
    rs = td.Resize(dev, (src[1], src[0]), (dst[1], dst[0]))
    x = torch.from_numpy(rand_f((*src, 3), 71) * 255).to(dev).to(dtype)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = rs.process(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, rs.process(x))
    x.copy_(torch.from_numpy(rand_f((*src, 3), 72) * 255).to(dev).to(dtype))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, rs.process(x))


# ------------------------------------------------------------------ 7. pipeline
def _processor(td, dev, w, h, resize_width, transforms):
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True,
                                       tone_mapping=ToneMapper.reinhard, resize_width=resize_width)
    cam = CameraSettings(name='cam', image_size=(w, h), padding=0, white_balance=(1.4, 1.0, 1.3), image_processing=settings, transform=transforms)
    return ImageProcessor.from_camera_settings(cam, dev)


def _packed(td, dev, w, h, seed, gain=1.0):
    from torch_darktable.synthetic import synthetic_bayer
    bayer = (synthetic_bayer(h, w, seed=seed, device='cpu') * gain).clamp(0, 1)
    return td.encode12_float(bayer.to(dev).reshape(-1))


def test_process_resized_is_transform_of_resize_of_process(td, dev):
    from torch_darktable.pipeline import ImageTransform
    from torch_darktable.pipeline.transform import transform, transformed_size
    w, h, rw = 256, 192, 100
    packed = _packed(td, dev, w, h, 81)
    for t in (ImageTransform.none, ImageTransform.rotate_90, ImageTransform.flip_horiz):
        proc = _processor(td, dev, w, h, rw, t)
        assert proc.final_size == (100, 75)
        plain = _processor(td, dev, w, h, rw, ImageTransform.none)
        out = proc.process_resized(packed, 'cam')
        tw, th = transformed_size(proc.final_size, t)
        assert tuple(out.shape) == (th, tw, 3) and out.dtype == torch.uint8 and out.is_contiguous(), (t, out.shape)
        before = plain.process(packed, 'cam')                      # ignores resize_width: the full-size frame, not oriented
        assert tuple(before.shape) == (h, w, 3)
        want = transform(td.Resize(dev, (w, h), proc.final_size).process(before), t)
        assert torch.equal(out, want), t
        # and `process` of the same processor still returns the full-size oriented frame
        full = _processor(td, dev, w, h, rw, t).process(packed, 'cam')
        assert tuple(full.shape) == (*transformed_size((w, h), t)[::-1], 3) and torch.equal(full, transform(before, t))
    check_u8(td, dev, before.cpu().numpy(), (75, 100), 'pipeline frame ')


def test_process_resized_without_resize_width_is_process(td, dev):
    from torch_darktable.pipeline import ImageTransform
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 82)
    a = _processor(td, dev, w, h, 0, ImageTransform.rotate_90)
    b = _processor(td, dev, w, h, 0, ImageTransform.rotate_90)
    assert a.resize_workspace is None
    assert torch.equal(a.process_resized(packed, 'cam'), b.process(packed, 'cam'))
    sets = {'left': packed, 'right': _packed(td, dev, w, h, 83)}
    ra, rb = a.process_image_set_resized(sets), b.process_image_set(sets)
    assert list(ra) == list(rb) and all(torch.equal(ra[k], rb[k]) for k in ra)


def test_resized_calls_keep_the_moving_averages_of_process(td, dev):
    from torch_darktable.pipeline import ImageTransform
    w, h = 256, 192
    frames = [_packed(td, dev, w, h, 84), _packed(td, dev, w, h, 85, gain=0.5)]   # the second is darker: the EMA decides
    a = _processor(td, dev, w, h, 64, ImageTransform.none)
    b = _processor(td, dev, w, h, 64, ImageTransform.none)
    for f in frames:
        small, full = a.process_resized(f, 'cam'), b.process(f, 'cam')
        assert tuple(small.shape) == (48, 64, 3) and tuple(full.shape) == (h, w, 3)
        assert torch.equal(a.bounds, b.bounds) and torch.equal(a.metrics, b.metrics)
        assert torch.equal(small, td.Resize(dev, (w, h), (64, 48)).process(full))


def test_update_settings_rebuilds_the_scaler(td, dev):
    from torch_darktable.pipeline import ImageTransform
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 86)
    proc = _processor(td, dev, w, h, 64, ImageTransform.none)
    first = proc.resize_workspace
    assert first.output_size == (64, 48)
    proc.update_settings(proc.settings.model_copy(update={'tone_gamma': proc.settings.tone_gamma * 0.9}))
    assert proc.resize_workspace is first                       # another setting: kept
    proc.update_settings(proc.settings.model_copy(update={'resize_width': 128}))
    assert proc.resize_workspace.output_size == (128, 96)
    assert tuple(proc.process_resized(packed, 'cam').shape) == (96, 128, 3)
    proc.update_settings(proc.settings.model_copy(update={'resize_width': 0}))
    assert proc.resize_workspace is None and tuple(proc.process_resized(packed, 'cam').shape) == (h, w, 3)
    proc.update_settings(proc.settings.model_copy(update={'resize_width': 8}))    # 32:1: only the resized call refuses
    assert tuple(proc.process(packed, 'cam').shape) == (h, w, 3)
    with pytest.raises(ValueError, match='ratio'):
        proc.process_resized(packed, 'cam')
