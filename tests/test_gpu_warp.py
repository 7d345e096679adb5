"""GPU: the parametric warp (torch_darktable.Warp, include/tdk_hip_warp.h) against the float32 restatement of its specification,
`warp_ref` / `coords_ref` of tests/test_warp_spec.py (whose float64 twin is pinned there to torch's CPU grid_sample).

The criterion is bit equality, for float32, float16 and uint8 alike: the restatement uses only correctly rounded float32
operations in the order of the specification, and the library is built without contraction.  A differing bit is a finding to
explain (a contracted multiply-add, a division that is not correctly rounded, a reordered sum), not a tolerance to widen.  Floats
are compared as their bit patterns, so NaN positions and the sign of zero count too.

Every parity check prints its figures (pytest -s) before it asserts."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('warp_spec', Path(__file__).resolve().parent / 'test_warp_spec.py')
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)
warp_ref, coords_ref, split_ref, homography_map, camera_map = spec.warp_ref, spec.coords_ref, spec.split_ref, spec.homography_map, spec.camera_map

NP = {'float32': np.float32, 'float16': np.float16, 'uint8': np.uint8}
TILE_W, TILE_H, BOX = 32, 16, 2048   # csrc/warp.hip: the output tile of a workgroup and the source pixels it can stage


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if NP[dtype] == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.random(shape).astype(NP[dtype])


def bits(a):
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements into a larger buffer."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


def run(td, dev, img, m, out_size, interp='bicubic', border='constant', fill=0.0, direct=False, offset=0):
    t = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    if offset:
        t = at_offset(t, offset)
    wp = td.Warp(dev, (img.shape[1], img.shape[0]), out_size, m, interpolation=interp, border=border, fill=fill)
    out = wp.process(t, direct=direct)
    assert tuple(out.shape) == (out_size[1], out_size[0], img.shape[2]) and out.dtype == t.dtype and out.is_contiguous()
    return out.cpu().numpy()


def check(td, dev, img, m, out_size, interp='bicubic', border='constant', fill=0.0, what='', offset=0, both_paths=False):
    want = warp_ref(img, m, out_size, interp, border, fill)
    got = run(td, dev, img, m, out_size, interp, border, fill, offset=offset)
    differ = bits(got) != bits(want)
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f'warp {what}{img.shape} {img.dtype} -> {out_size} {interp}/{border}: {int(differ.sum())} of {differ.size} values differ in a bit, '
          f'largest difference {worst:.3e}')
    assert not differ.any(), (what, img.shape, str(img.dtype), interp, border, int(differ.sum()), worst)
    if both_paths:
        direct = run(td, dev, img, m, out_size, interp, border, fill, direct=True, offset=offset)
        assert np.array_equal(bits(direct), bits(got)), (what, 'TDK_WARP_DIRECT differs from flags = 0')
    return got


def check_coordinates(td, dev, m, out_size):
    sx, sy, outside = coords_ref(m, *out_size)
    want = np.stack([np.where(outside, np.float32(np.nan), sx), np.where(outside, np.float32(np.nan), sy)], axis=-1)
    xy = td.Warp(dev, (8, 8), out_size, m).coordinates()
    assert tuple(xy.shape) == (out_size[1], out_size[0], 2) and xy.dtype == torch.float32
    got = xy.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    differ = (bits(got) != bits(want)) & ~np.isnan(want)
    print(f'warp coordinates -> {out_size}: {int(differ.sum())} of {differ.size} differ in a bit, {int(outside.sum())} pixels outside')
    assert not differ.any()


def tile_paths(m, src_size, out_size, interp):
    """(staged, direct, empty) tile counts by the rule of csrc/warp.hip: a tile is staged when the bounding box of its taps,
    clamped into the frame, holds at most BOX source pixels.  Only used to show that a case exercises what it claims to."""
    sw, sh = src_size
    sx, sy, outside = coords_ref(m, *out_size)
    n = 4 if interp == 'bicubic' else 2
    ix, _ = split_ref(np.where(outside, np.float32(0), sx), sw)
    iy, _ = split_ref(np.where(outside, np.float32(0), sy), sh)
    first = 1 if n == 4 else 0
    x0, x1 = np.clip(ix - first, 0, sw - 1), np.clip(ix - first + n - 1, 0, sw - 1)
    y0, y1 = np.clip(iy - first, 0, sh - 1), np.clip(iy - first + n - 1, 0, sh - 1)
    staged = direct = empty = 0
    for ty in range(0, out_size[1], TILE_H):
        for tx in range(0, out_size[0], TILE_W):
            s = (slice(ty, ty + TILE_H), slice(tx, tx + TILE_W))
            ok = ~outside[s]
            if not ok.any():
                empty += 1
                continue
            bw, bh = x1[s][ok].max() - x0[s][ok].min() + 1, y1[s][ok].max() - y0[s][ok].min() + 1
            if bw * bh <= BOX:
                staged += 1
            else:
                direct += 1
    return staged, direct, empty


# ------------------------------------------------------------------ 1. identity and translation
@pytest.mark.parametrize('interp', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'uint8'])
@pytest.mark.parametrize('channels', [1, 3])
def test_identity_map_returns_the_input(td, dev, channels, dtype, interp):
    img = image((29, 37, channels), dtype, 1)
    for border in ('constant', 'replicate'):
        got = run(td, dev, img, homography_map(np.eye(3)), (37, 29), interp, border, 9.0)
        assert np.array_equal(bits(got), bits(img)), (channels, dtype, interp, border)


@pytest.mark.parametrize('interp', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'uint8'])
def test_integer_translation_shifts_the_input(td, dev, dtype, interp):
    """Output (u, v) reads source (u + 3, v - 2): the uncovered band (two rows on top, three columns on the right) is fill = 7
    under constant and the edge values under replicate."""
    img = image((29, 37, 3), dtype, 2)
    m = homography_map([[1, 0, 3], [0, 1, -2], [0, 0, 1]])
    want = np.full_like(img, 7)
    want[2:, :34] = img[:27, 3:]
    got = check(td, dev, img, m, (37, 29), interp, 'constant', 7.0, 'translation ')
    assert np.array_equal(bits(got), bits(want))
    want = img[np.clip(np.arange(29) - 2, 0, 28)][:, np.clip(np.arange(37) + 3, 0, 36)]
    got = check(td, dev, img, m, (37, 29), interp, 'replicate', 7.0, 'translation ')
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------ 2. undistortion
UNDISTORT = {'same': ((203, 151), camera_map((203, 151))), 'new_camera': ((160, 120), camera_map((203, 151), (160, 120), zoom=0.9))}


@pytest.mark.parametrize('border', ['constant', 'replicate'])
@pytest.mark.parametrize('interp', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'uint8'])
@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('case', ['same', 'new_camera'])
def test_undistort_is_bit_equal_to_the_restatement(td, dev, case, channels, dtype, interp, border):
    out_size, m = UNDISTORT[case]
    img = image((151, 203, channels), dtype, 3)
    check(td, dev, img, m, out_size, interp, border, 7.0 if dtype == 'uint8' else 0.25, f'undistort {case} ', both_paths=True)


def test_undistort_from_the_front_end_equals_the_map(td, dev):
    K = np.array([[146.2, 0, 101.1], [0, 146.0, 75.9], [0, 0, 1]])
    dist = [-0.12, 0.09, 8e-4, -5e-4, -0.02]
    wp = td.Warp.undistort(dev, (203, 151), K, dist, interpolation='bilinear', border='replicate')
    img = image((151, 203, 3), 'uint8', 4)
    got = wp.process(torch.from_numpy(img).to(dev)).cpu().numpy()
    assert np.array_equal(got, warp_ref(img, spec.undistort_map(K, dist), (203, 151), 'bilinear', 'replicate', 0.0))
    assert np.array_equal(wp.map, np.asarray(spec.undistort_map(K, dist), dtype=np.float32))


@pytest.mark.parametrize('case', ['same', 'new_camera'])
def test_coordinates_are_bit_equal_to_the_restatement(td, dev, case):
    out_size, m = UNDISTORT[case]
    check_coordinates(td, dev, m, out_size)


# ------------------------------------------------------------------ 3. perspective with a horizon; minification
def horizon_map():
    """Rotation by 30 degrees about the output centre and a tilt whose horizon (Z = 0) lies between output rows 80 and 81."""
    a = np.deg2rad(30.0)
    to_centre = np.array([[1, 0, -63.5], [0, 1, -47.5], [0, 0, 1]])
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    back = np.array([[1.3, 0, 90.0], [0, 1.3, 69.5], [0, 0, 1]])
    H = back @ rot @ to_centre
    H[2] = [0.0, -1.0 / 80.5, 1.0]
    return homography_map(H)


@pytest.mark.parametrize('border', ['constant', 'replicate'])
@pytest.mark.parametrize('interp', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'uint8'])
def test_perspective_with_the_horizon_inside_the_output(td, dev, dtype, interp, border):
    m, src, out = horizon_map(), (181, 140), (128, 96)
    _, _, outside = coords_ref(m, *out)
    assert outside[81:].all() and not outside[:81].any()
    staged, direct, empty = tile_paths(m, src, out, interp)
    print(f'horizon: {staged} staged, {direct} direct, {empty} empty tiles')
    assert staged > 0 and direct > 0   # both sampling paths in one launch
    img = image((140, 181, 3), dtype, 5)
    fill = 7.0 if dtype == 'uint8' else 0.25
    got = check(td, dev, img, m, out, interp, border, fill, 'horizon ', both_paths=True)
    assert (got[81:] == NP[dtype](fill)).all()


def test_coordinates_beyond_the_horizon_are_nan(td, dev):
    check_coordinates(td, dev, horizon_map(), (128, 96))


@pytest.mark.parametrize('interp', ['bilinear', 'bicubic'])
def test_uniform_minification_samples_directly(td, dev, interp):
    m, src, out = homography_map(np.diag([40.0, 40.0, 1.0])), (1200, 900), (30, 22)
    assert tile_paths(m, src, out, interp) == (0, 2, 0)   # either tile's box spans the source's width: no tile is staged
    img = image((900, 1200, 3), 'uint8', 6)
    check(td, dev, img, m, out, interp, 'constant', 7.0, 'minify 1:40 ', both_paths=True)


# ------------------------------------------------------------------ 4. orientations
@pytest.mark.parametrize('dtype', ['uint8', 'float16'])
def test_from_transform_equals_pipeline_transform(td, dev, dtype):
    from torch_darktable.pipeline.transform import ImageTransform, transform, transformed_size

    img = torch.from_numpy(image((41, 53, 3), dtype, 7)).to(dev)
    for t in ImageTransform:
        for interp in ('bilinear', 'bicubic'):
            wp = td.Warp.from_transform(dev, (53, 41), t, interpolation=interp, fill=200.0)
            got = wp.process(img)
            assert wp.output_size == transformed_size((53, 41), t)
            assert torch.equal(got, transform(img, t)), (t, interp)


# ------------------------------------------------------------------ 5. large coordinates, misaligned frames
def test_large_coordinates_float16_strip(td, dev):
    img = image((24, 4096, 3), 'float16', 8)
    m = camera_map((4096, 24))
    for interp in ('bilinear', 'bicubic'):
        check(td, dev, img, m, (4096, 24), interp, 'replicate', 0.0, 'f = 2950 strip ', both_paths=True)
    check_coordinates(td, dev, m, (4096, 24))


def test_widest_frame_shifted_by_half_a_pixel(td, dev):
    img = image((2, 65535, 1), 'uint8', 9)
    m = homography_map([[1, 0, 0.5], [0, 1, 0], [0, 0, 1]])
    for border in ('constant', 'replicate'):
        check(td, dev, img, m, (65535, 2), 'bilinear', border, 7.0, '65535 wide ', both_paths=True)


@pytest.mark.parametrize('interp', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('dtype', ['float16', 'uint8'])
def test_frames_one_element_into_a_buffer(td, dev, dtype, channels, interp):
    out_size, m = UNDISTORT['same']
    img = image((151, 203, channels), dtype, 10)
    check(td, dev, img, m, out_size, interp, 'constant', 7.0, 'offset view ', offset=1, both_paths=True)


# ------------------------------------------------------------------ 6. determinism, capture, errors
def test_two_calls_give_equal_bits(td, dev):
    out_size, m = UNDISTORT['new_camera']
    for dtype in ('float32', 'float16', 'uint8'):
        x = torch.from_numpy(image((151, 203, 3), dtype, 11)).to(dev)
        wp = td.Warp(dev, (203, 151), out_size, m)
        a, b = wp.process(x), wp.process(x)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize('dtype', ['float32', 'float16', 'uint8'])
def test_graph_capture_from_the_first_call(td, dev, dtype):
    """A fresh object captured on one stream without a warm-up call; the replay equals the eager result bit for bit, also after
    the input buffer's contents change."""
    m = camera_map((211, 157), (173, 131), zoom=0.95)
    wp = td.Warp(dev, (211, 157), (173, 131), m, border='replicate')
    x = torch.from_numpy(image((157, 211, 3), dtype, 12)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = wp.process(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, wp.process(x))
    x.copy_(torch.from_numpy(image((157, 211, 3), dtype, 13)).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, wp.process(x))
    assert np.array_equal(captured.cpu().numpy(), warp_ref(x.cpu().numpy(), m, (173, 131), 'bicubic', 'replicate', 0.0))


def test_error_handling_matches_resize(td, dev):
    wp = td.Warp(dev, (64, 48), (16, 12), homography_map(np.eye(3)))
    rs = td.Resize(dev, (64, 48), (16, 12))
    bad = [torch.zeros(48, 60, 3, device=dev), torch.zeros(48, 64, 2, device=dev), torch.zeros(48, 64, 3, device=dev, dtype=torch.int32),
           torch.zeros(48, 64, 3, device=dev, dtype=torch.float64), torch.zeros(48, 64, 6, device=dev)[:, :, ::2],
           torch.zeros(64, 48, 3, device=dev).transpose(0, 1), torch.zeros(48, 64, 3)]
    for x in bad:
        with pytest.raises(Exception) as theirs:
            rs.process(x)
        with pytest.raises(theirs.type):
            wp.process(x)
    assert tuple(wp.process(torch.zeros(48, 64, 3, device=dev)).shape) == (12, 16, 3)
