"""CPU-only: the header include/tdk_hip_deconv.h (capture sharpening) -- it parses to exactly its six declarations (exports and the
ctypes table: tests/test_header_abi.py), its constants and formulas are the ones the restatement uses, its source is part of the
build's source hash, every argument error of tdk_deconv is reported on the host before any HIP call, the workspace, LDS and
fused-count queries answer what the documents say, and the Python front-end torch_darktable.Deconvolve and the pipeline property
raise the error types of the other operators."""

import ctypes
import inspect
import re
from pathlib import Path

import pytest

import deconv_spec as spec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_deconv.h'
EXPECTED = ['tdk_deconv', 'tdk_deconv_abi_version', 'tdk_deconv_fused_iterations', 'tdk_deconv_lds_bytes', 'tdk_deconv_weights', 'tdk_deconv_workspace_bytes']
F32, F16, U8 = 0, 1, 2
MASK = 1


def fuse(f):
    return f << 8


def test_header_declares_the_deconvolution_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for name, value in (('ABI_VERSION', 1), ('MASK', 1), ('FUSE_SHIFT', 8), ('FUSE_MASK', 3840), ('MAX_RADIUS', 6), ('MAX_ITERATIONS', 50), ('MAX_FUSED', 4), ('TILE', 32)):
        assert re.search(rf'#define TDK_DECONV_{name} {value}\b', text), name
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_deconv'] == ('int', ['const void* src', 'void* dst', 'float* mask_out', 'void* workspace', 'int width', 'int height', 'int channels', 'int dtype',
                                           'const float* weights', 'int radius', 'int iterations', 'float threshold', 'float max_gain', 'const float* luma', 'int flags',
                                           'tdk_stream_t stream'])
    assert decls['tdk_deconv_weights'] == ('int', ['float sigma', 'float* weights', 'int* radius'])
    assert decls['tdk_deconv_workspace_bytes'] == ('size_t', ['int width', 'int height', 'int radius', 'int iterations'])
    assert decls['tdk_deconv_lds_bytes'] == ('size_t', ['int channels', 'int dtype', 'int radius', 'int flags'])
    assert decls['tdk_deconv_fused_iterations'] == ('int', ['int radius'])
    assert decls['tdk_deconv_abi_version'] == ('int', [])
    for ret, params in decls.values():   # scalar parameters stay within int, float and size_t
        assert all('*' in p or p.split()[0] in ('int', 'float', 'size_t', 'tdk_stream_t') for p in params), params
    for formula in ('pos(v) = v > 0 ? v : +0', 'Y = pos((l0*r + l1*g) + l2*b)', 'Y = pos(x)', 'o = fmaxf(Y, TINY)', 'TINY = 2^-20', 'h = w[0]*s[0]',
                    'h = h + w[k]*(s[-k] + s[+k])', 'u_0 = o', 'b   = G(u_{k-1})', 'q   = o / fmaxf(b, TINY)', 'c   = G(q)', 'u_k = u_{k-1} * c',
                    'd  = sqrtf(hi) - sqrtf(lo)', 'it = 1 / t', 'e  = fminf(fmaxf((d - t) * it, 0), 1)', 'm  = (e*e) * (3 - 2*e)', 'Yn = o + m*(u_N - o)',
                    'g  = fminf(fmaxf(Yn / o, 1 / G), G)', 'out_c = x_c * g', 'N == 0 stores x_c itself'):
        assert formula in text, formula
    assert (_native.TDK_DECONV_MASK, _native.TDK_DECONV_FUSE_SHIFT, _native.TDK_DECONV_FUSE_MASK) == (1, 8, 3840) == (spec.MASK, spec.FUSE_SHIFT, spec.FUSE_MASK)
    assert (_native.TDK_DECONV_MAX_RADIUS, _native.TDK_DECONV_MAX_ITERATIONS, _native.TDK_DECONV_MAX_FUSED, _native.TDK_DECONV_TILE) == (6, 50, 4, 32)
    assert (spec.MAX_RADIUS, spec.MAX_ITERATIONS, spec.MAX_FUSED, spec.TILE) == (6, 50, 4, 32) and float(spec.TINY) == 2.0 ** -20
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_deconv.h']
    assert rows == [('tdk_hip_deconv.h', _native.DECONV_SIGNATURES, 'tdk_deconv_abi_version', 1, 'deconvolution ABI')]
    assert _native.ABI_VERSIONS['tdk_deconv_abi_version'] == (1, 'deconvolution ABI')
    assert sorted(_native.DECONV_SIGNATURES) == EXPECTED and _native.lib.tdk_deconv_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'deconv.hip') in build._inputs()
    assert [h.name for h in build.HEADERS] == [row[0] for row in _native.HEADERS]


def test_weights_are_the_restatements(td):
    from torch_darktable._native import lib

    buf, radius = (ctypes.c_float * 7)(), ctypes.c_int(-1)
    for sigma in (0.3, 0.45, 0.7, 1.0, 1.2, 1.7, 2.0):
        buf[:] = [9.0] * 7
        assert lib.tdk_deconv_weights(sigma, buf, ctypes.byref(radius)) == 0
        taps = spec.gaussian_taps(sigma)
        assert radius.value == len(taps) - 1 and tuple(buf[: len(taps)]) == tuple(float(t) for t in taps) and all(v == 0.0 for v in buf[len(taps):])
    for sigma in (0.29, 2.01, 0.0, -1.0, float('nan'), float('inf')):
        assert lib.tdk_deconv_weights(sigma, buf, ctypes.byref(radius)) == 1 and b'tdk_deconv_weights: sigma must lie in [0.3, 2]' in lib.tdk_last_error()
    assert lib.tdk_deconv_weights(0.7, None, ctypes.byref(radius)) == 1 and b'null pointer' in lib.tdk_last_error()
    assert lib.tdk_deconv_weights(0.7, buf, None) == 1 and b'null pointer' in lib.tdk_last_error()


def test_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    taps = (ctypes.c_float * 4)(*spec.gaussian_taps(0.7))
    rec709 = (ctypes.c_float * 3)(0.2126, 0.7152, 0.0722)
    names = ['src', 'dst', 'm', 'ws', 'w', 'h', 'channels', 'dtype', 'weights', 'radius', 'iterations', 'threshold', 'max_gain', 'luma', 'flags', 'stream']
    args = [fake, fake + (1 << 24), fake + (2 << 24), fake + (3 << 24), 640, 480, 3, F32, taps, 3, 8, 0.02, 4.0, rec709, MASK, None]

    def fails(needle, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        assert lib.tdk_deconv(*a) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())
        assert lib.tdk_last_error().startswith(b'tdk_deconv:')

    for k in ('src', 'dst', 'weights', 'luma'):
        fails(b'null pointer', **{k: None})
    fails(b'null pointer (workspace', ws=None)
    for k in ('w', 'h'):
        for v in (0, -2, 65536):
            fails(b'frame size', **{k: v})
    for c in (0, 2, 4, -1):
        fails(b'channels must be 1 or 3', channels=c)
    for d in (U8, 3, -1):
        fails(b'dtype', dtype=d)
    for r in (0, -1, 7, 64):
        fails(b'radius must be 1..6', radius=r, weights=(ctypes.c_float * 65)(*([0.01] * 65)))
    for k, bad in enumerate((float('nan'), float('inf'), -0.5, -1e-9)):
        w = [float(t) for t in spec.gaussian_taps(0.7)]
        w[k] = bad
        fails(f'weights[{k}]'.encode(), weights=(ctypes.c_float * 4)(*w))
    for n in (-1, 51, 1 << 20):
        fails(b'iterations must be 0..50', iterations=n)
    for t in (0.0, -0.02, float('nan'), float('inf'), 1e-50):   # (1e-50 is 0 as a float32)
        fails(b'threshold must be finite and > 0', threshold=t)
    for g in (0.99, 16.5, 0.0, -4.0, float('nan'), float('inf')):
        fails(b'max_gain must lie in [1, 16]', max_gain=g)
    for k, bad in enumerate((float('nan'), float('inf'), -0.5)):
        l = [0.2126, 0.7152, 0.0722]
        l[k] = bad
        fails(f'luma[{k}]'.encode(), luma=(ctypes.c_float * 3)(*l))
    for f in (2, 4, 128, MASK | 4096, -1, 1 << 30):
        fails(b'reserved', flags=f)
    for f in (3, 5, 8, 15):   # a fused count that was not built
        fails(b'fused count', flags=MASK | fuse(f))
    fails(b'fused count', flags=fuse(4))   # F = 4 takes radii up to 2
    fails(b'fused count', flags=fuse(2), radius=5, weights=(ctypes.c_float * 6)(*([0.1] * 6)))
    fails(b'mask_out must be aligned', m=fake + (2 << 24) + 2)
    # overlap, in bytes of the dtype
    frame, plane = 640 * 480 * 3 * 4, 640 * 480 * 4
    for dst in (fake, fake + 64, fake - frame + 4, fake + frame - 4):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + frame // 2 - 2, dtype=F16)
    for m in (fake + 128, fake + frame - 4, fake + (1 << 24) - plane + 4, fake + (1 << 24) + frame - 4):
        fails(b'mask_out overlaps src or dst', m=m)
    for ws in (fake + 16, fake + (1 << 24) - 64, fake + (2 << 24) + 4, fake + (2 << 24) + plane - 8, fake + (2 << 24) - 2 * plane):
        fails(b'the workspace overlaps', ws=ws)
    # a threshold that is not read, a null mask_out and a null workspace of a one-launch call pass every check -- and would reach the launch: not made here


def test_workspace_lds_and_fused_queries(td):
    from torch_darktable._native import lib

    # F per radius: measured on the MI355X (profiles/r25/deconv_bench.txt), F = 1 is the fastest everywhere
    assert [lib.tdk_deconv_fused_iterations(r) for r in range(-1, 9)] == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0]
    for w, h in ((640, 480), (641, 481), (1, 1), (65535, 65535)):
        for radius in (1, 3, 6):
            fused = lib.tdk_deconv_fused_iterations(radius)
            for iterations in (0, 1, fused, fused + 1, 2 * fused, 2 * fused + 1, 50):
                want = spec.workspace_bytes(w, h, spec.launches(iterations, fused))
                assert lib.tdk_deconv_workspace_bytes(w, h, radius, iterations) == want, (w, h, radius, iterations)
    assert lib.tdk_deconv_workspace_bytes(640, 480, 3, 0) == lib.tdk_deconv_workspace_bytes(640, 480, 3, 1) == 0   # one launch
    assert lib.tdk_deconv_workspace_bytes(640, 480, 3, 2) == 640 * 480 * 4 + 16 and lib.tdk_deconv_workspace_bytes(640, 480, 3, 8) == 2 * 640 * 480 * 4 + 16
    assert lib.tdk_deconv_workspace_bytes(3, 3, 1, 3) == 2 * 48 + 16   # planes start on 16 bytes
    for bad in ((0, 480, 3, 8), (640, 65536, 3, 8), (640, 480, 0, 8), (640, 480, 7, 8), (640, 480, 3, -1), (640, 480, 3, 51)):
        assert lib.tdk_deconv_workspace_bytes(*bad) == 0, bad
    for channels in (1, 3):
        for tag in (F32, F16):
            assert lib.tdk_deconv_lds_bytes(channels, tag, 3, MASK) == lib.tdk_deconv_lds_bytes(channels, tag, 6, fuse(1)) == 4 * 4 * 56 * 56
            assert lib.tdk_deconv_lds_bytes(channels, tag, 4, fuse(2)) == lib.tdk_deconv_lds_bytes(channels, tag, 2, MASK | fuse(4)) == 4 * 4 * 64 * 64 == 65536
    for bad in ((2, F32, 3, 0), (3, U8, 3, 0), (3, -1, 3, 0), (3, F32, 0, 0), (3, F32, 7, 0), (3, F32, 3, 2), (3, F32, 3, fuse(4)), (3, F32, 5, fuse(2)), (3, F32, 3, fuse(3)),
                (3, F32, 3, -1)):
        assert lib.tdk_deconv_lds_bytes(*bad) == 0, bad


def test_package_exports_the_deconvolution(td):
    import torch_darktable

    assert torch_darktable.Deconvolve is torch_darktable.deconvolve.Deconvolve
    assert 'Deconvolve' in torch_darktable.__all__ and 'deconvolve' in torch_darktable.__all__
    assert torch_darktable.deconvolve.__all__ == ['Deconvolve'] and torch_darktable.sharpen.__all__ == ['Sharpen']
    D = torch_darktable.Deconvolve
    for name in ('process', 'mask', 'workspace_bytes', 'lds_bytes', 'from_weights'):
        assert callable(getattr(D, name)), name
    for name in ('radius', 'taps', 'fused_iterations', 'launches', 'image_size'):
        assert isinstance(getattr(D, name), property), name
    params = inspect.signature(D.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'sigma', 'iterations', 'threshold', 'max_gain', 'weights']
    assert [params[k].default for k in list(params)[3:]] == [0.7, 8, 0.02, 4.0, None]
    params = inspect.signature(D.from_weights).parameters
    assert list(params) == ['device', 'image_size', 'taps', 'iterations', 'threshold', 'max_gain', 'weights']
    assert [params[k].default for k in list(params)[3:]] == [8, 0.02, 4.0, None]
    params = inspect.signature(D.process).parameters
    assert list(params) == ['self', 'image', 'return_mask'] and params['return_mask'].default is False
    assert list(inspect.signature(D.mask).parameters) == ['self', 'image']
    assert list(inspect.signature(D.lds_bytes).parameters) == ['self', 'dtype', 'channels'] and list(inspect.signature(D.workspace_bytes).parameters) == ['self']
    assert D.TILE == (32, 32)


def test_pipeline_takes_the_stage_as_a_property_only(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.camera_settings import CameraSettings

    assert not any('capture' in name or 'deconv' in name for name in inspect.signature(ImageProcessor.__init__).parameters)
    assert not any('capture' in name or 'deconv' in name for name in inspect.signature(ImageProcessor.from_camera_settings).parameters)
    assert list(inspect.signature(ImageProcessor.__init__).parameters)[-1] == 'raw_correction'
    for model in (ImageProcessingSettings, CameraSettings):
        assert not any('capture' in name or 'deconv' in name for name in model.model_fields), model
    assert isinstance(ImageProcessor.capture_sharpen, property) and ImageProcessor.capture_sharpen.fset is not None
    assert ImageProcessor._capture_sharpen is None   # the class-level default
    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    # an object made without the constructor has the slot through the class: the property needs the size only
    p = ImageProcessor.__new__(ImageProcessor)
    p.image_size = (64, 48)
    assert '_capture_sharpen' not in vars(p) and p.capture_sharpen is None
    for bad in (object(), 3, 'rl', td.Sharpen(cuda), td.Dehaze(cuda, (64, 48))):
        with pytest.raises(TypeError, match='capture_sharpen must be a Deconvolve or None'):
            p.capture_sharpen = bad
    for size in ((32, 48), (64, 50), (48, 64)):
        with pytest.raises(ValueError, match=rf'capture_sharpen is for {size[0]}x{size[1]}, the processor for 64x48'):
            p.capture_sharpen = td.Deconvolve(cuda, size)
    assert p.capture_sharpen is None
    d = td.Deconvolve(cuda, (64, 48))
    p.capture_sharpen = d
    assert p.capture_sharpen is d and ImageProcessor._capture_sharpen is None
    p.capture_sharpen = None
    assert p.capture_sharpen is None
    source = inspect.getsource(ImageProcessor._process_frames)
    assert source.index('self.chroma_denoise.process(img)') < source.index('self._capture_sharpen.process') < source.index('self.color.process')
    assert source.index('self.color.process') < source.index('self._dehaze.process') < source.index('self._tone_equalizer.process')   # nothing else moved


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)
    D = td.Deconvolve
    with pytest.raises(ValueError, match='CUDA'):
        D(torch.device('cpu'), (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions must be 1'):
            D(cuda, size)
    for sigma in (0.29, 2.5, 0.0, float('nan')):
        with pytest.raises(ValueError, match='sigma must lie in'):
            D(cuda, (64, 48), sigma=sigma)
    for iterations in (-1, 51, 2.5):
        with pytest.raises(ValueError, match='iterations must be'):
            D(cuda, (64, 48), iterations=iterations)
    for threshold in (0.0, -0.1, float('nan'), float('inf'), 1e-50):
        with pytest.raises(ValueError, match='threshold must be'):
            D(cuda, (64, 48), threshold=threshold)
    for gain in (0.5, 16.5, float('nan')):
        with pytest.raises(ValueError, match='max_gain must lie in'):
            D(cuda, (64, 48), max_gain=gain)
    for weights in ((1, 1), (1, 1, -1), (1, float('nan'), 1)):
        with pytest.raises(ValueError, match='weights must be'):
            D(cuda, (64, 48), weights=weights)
    for taps in ((1.0,), (0.1,) * 8, (0.5, -0.25), (0.5, float('nan'))):
        with pytest.raises(ValueError, match='taps must'):
            D.from_weights(cuda, (64, 48), taps)

    d = D(cuda, (64, 48), sigma=0.7, iterations=5, threshold=0.03, max_gain=2.0)
    assert (d.width, d.height, d.image_size, d.radius, d.iterations, d.max_gain) == (64, 48, (64, 48), 3, 5, 2.0)
    assert d.sigma == ctypes.c_float(0.7).value and d.threshold == ctypes.c_float(0.03).value
    assert d.taps == tuple(float(t) for t in spec.gaussian_taps(0.7))
    assert d.weights == tuple(ctypes.c_float(v).value for v in (0.2126, 0.7152, 0.0722))
    assert d.fused_iterations == 1 and d.launches == 5 and d.workspace_bytes() == 2 * 64 * 48 * 4 + 16 == spec.workspace_bytes(64, 48, 5)
    assert repr(d) == 'Deconvolve(64x48, sigma=0.7, radius=3, iterations=5, threshold=0.03, max_gain=2)'
    assert 0 < d.lds_bytes(torch.float16, 1) <= 65536 and d.lds_bytes(torch.float32, 3) == d.lds_bytes(torch.float16, 1)
    assert d.lds_bytes(torch.uint8, 3) == 0 and d.lds_bytes(torch.float32, 2) == 0
    d.fused_iterations = 2
    assert d.fused_iterations == 2 and d.launches == 3 and d.lds_bytes() == 65536 and d.workspace_bytes() == 2 * 64 * 48 * 4 + 16
    for bad in (3, 4, 8):   # 4 does not take radius 3
        with pytest.raises(ValueError, match='fused_iterations must be'):
            d.fused_iterations = bad
    d.fused_iterations = None
    assert d.fused_iterations == 1
    off = D(cuda, (64, 48), threshold=None, iterations=0)
    assert off.threshold is None and off.launches == 1 and off.workspace_bytes() == 0 and 'threshold=None' in repr(off)
    own = D.from_weights(cuda, (64, 48), (0.5, 0.25), iterations=1)
    assert own.sigma is None and own.radius == 1 and own.taps == (0.5, 0.25) and own.workspace_bytes() == 0 and 'taps=(0.5, 0.25)' in repr(own)

    with pytest.raises(AssertionError, match='3 dimensions'):
        d.process(torch.zeros(48, 64))
    with pytest.raises(RuntimeError, match='expected'):
        d.process(torch.zeros(48, 32, 3))
    with pytest.raises(ValueError, match='channels must be 1 or 3'):
        d.process(torch.zeros(48, 64, 2))
    with pytest.raises(RuntimeError, match='CUDA'):
        d.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        d.mask(torch.zeros(48, 64, 1))
