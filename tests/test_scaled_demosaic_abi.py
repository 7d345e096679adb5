"""CPU-only: the header include/tdk_hip_scaled.h (the reduced-size demosaic) -- it parses to exactly its five declarations (exports
and the ctypes table: tests/test_header_abi.py), its constants and formulas are the ones the restatement uses, its source is part of
the build's source hash, every argument error of the two entry points is reported on the host before any HIP call (the status is
the one of an invalid argument, not of a failed launch, on a machine without a device too), the host queries answer what the
documents say, and the Python front end torch_darktable.ScaledDemosaic and the pipeline property raise the error types of the other
operators.  The stand-alone program tests/hip_unit/scaled_arguments_main.cpp makes the same calls for a run under a host sanitizer."""

import ctypes
import inspect
import re
from pathlib import Path

import pytest

import scaled_demosaic_spec as spec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_scaled.h'
EXPECTED = ['tdk_decode12_demosaic_scaled', 'tdk_demosaic_scaled', 'tdk_demosaic_scaled_lds_bytes', 'tdk_demosaic_scaled_tile', 'tdk_scaled_abi_version']
F32, F16, U8 = 0, 1, 2
INVALID_ARGUMENT = 1


def test_header_declares_the_scaled_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for name, value in (('ABI_VERSION', 1), ('MIN_RATIO', 2), ('MAX_RATIO', 16), ('MAX_TAPS', 32)):
        assert re.search(rf'#define TDK_SCALED_{name} {value}\b', text), name
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_demosaic_scaled'] == ('int', ['const void* src', 'void* dst', 'const float* gains', 'int width', 'int height', 'int out_width', 'int out_height',
                                                    'uint32_t pattern', 'int src_dtype', 'int dst_dtype', 'tdk_stream_t stream'])
    assert decls['tdk_decode12_demosaic_scaled'] == ('int', ['const uint8_t* packed', 'void* dst', 'const float* gains', 'int width', 'int height', 'int out_width',
                                                             'int out_height', 'uint32_t pattern', 'int ids_format', 'int dst_dtype', 'tdk_stream_t stream'])
    assert decls['tdk_demosaic_scaled_lds_bytes'] == ('size_t', ['int width', 'int height', 'int out_width', 'int out_height'])
    assert decls['tdk_demosaic_scaled_tile'] == ('int', ['int width', 'int height', 'int out_width', 'int out_height', 'int* tile_width', 'int* tile_height'])
    assert decls['tdk_scaled_abi_version'] == ('int', [])
    for formula in ('num(i, j) = 2*n_out*j + n_out - (2*i + 1)*n_in', 'iff   |num| < 2*n_in', 'w(i, j) = 1 - (float)|num| / (float)(2*n_in)', 'parity of a tap: j & 1',
                    '2*n_out <= n_in <= 16*n_out', 'acc = w*x for the first tap;   acc = fmaf(w, x, acc) for every further tap',
                    's = w for the first tap;       s = s + w for every further tap', 'acc = v*A_p[y][i] for the first tap;   acc = fmaf(v, A_p[y][i], acc)',
                    'N = B_qp                    D = Sy_q*Sx_p', 'N = B_0p1 + B_1p2           D = Sy_0*Sx_p1 + Sy_1*Sx_p2', 'out = N / D',
                    '(float)code * (1.0f / 4095.0f)', 'fminf(fmaxf(x*g, 0), 1)', 'g(n) = n*u / (1 - n*u), u = 2^-24, n = 2*(Tx + Ty + 1)',
                    'Pattern swap', 'Flat frames', 'Fused equals unfused', 'No mirror identity is claimed', 'at most 32 taps take part per axis', 'nothing is\n * clamped'):
        assert formula in text, formula
    assert (_native.TDK_SCALED_MIN_RATIO, _native.TDK_SCALED_MAX_RATIO, _native.TDK_SCALED_MAX_TAPS) == (2, 16, 32) == (spec.MIN_RATIO, spec.MAX_RATIO, spec.MAX_TAPS)
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_scaled.h']
    assert rows == [('tdk_hip_scaled.h', _native.SCALED_SIGNATURES, 'tdk_scaled_abi_version', 1, 'scaled demosaic ABI')]
    assert _native.ABI_VERSIONS['tdk_scaled_abi_version'] == (1, 'scaled demosaic ABI')
    assert sorted(_native.SCALED_SIGNATURES) == EXPECTED and _native.lib.tdk_scaled_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'scaled_demosaic.hip') in build._inputs()
    assert [h.name for h in build.HEADERS] == [row[0] for row in _native.HEADERS]


def test_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake, gap = 1 << 30, 1 << 24   # never dereferenced: every check below happens before anything touches device memory or a device
    names = ['src', 'dst', 'gains', 'w', 'h', 'ow', 'oh', 'pattern', 'kind', 'dst_dtype', 'stream']
    args = [fake, fake + gap, fake + 2 * gap, 640, 480, 160, 120, spec.RGGB, F32, F32, None]

    def fails(needle, fn='tdk_demosaic_scaled', **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        assert getattr(lib, fn)(*a) == INVALID_ARGUMENT and needle in lib.tdk_last_error(), (fn, change, lib.tdk_last_error())
        assert lib.tdk_last_error().startswith(fn.encode() + b':')

    for fn in ('tdk_demosaic_scaled', 'tdk_decode12_demosaic_scaled'):
        for k in ('src', 'dst'):
            fails(b'null pointer (src or dst)', fn, **{k: None})
        for k in ('w', 'h'):
            for v in (1, 0, -2, 65536):
                fails(b'mosaic size', fn, **{k: v})
        for k in ('ow', 'oh'):
            for v in (0, -1):
                fails(b'below 1x1', fn, **{k: v})
        fails(b'below 2:1 on an axis', fn, ow=321)
        fails(b'below 2:1 on an axis', fn, oh=241)
        fails(b'below 2:1 on an axis', fn, ow=640, oh=480)
        fails(b'beyond 16:1 on an axis', fn, ow=39)
        fails(b'beyond 16:1 on an axis', fn, oh=29)
        for p in (0, 1, 0x94949495, 0x94941616, 0xFFFFFFFF, 0x55555555):
            fails(b'invalid Bayer pattern', fn, pattern=p)
        for d in (U8, 3, -1):
            fails(b'unsupported dst dtype', fn, dst_dtype=d)
        fails(b'gains and dst overlap', fn, gains=fake + gap + 160 * 120 * 12 - 4)
        fails(b'src and dst overlap', fn, dst=fake)
        fails(b'ratio', fn, ow=39, gains=None)   # gains may be null: the same error with and without them
    for d in (U8, 3, -1):
        fails(b'unsupported src dtype', kind=d)
    fails(b'width must be even', 'tdk_decode12_demosaic_scaled', w=642 - 1, ow=160)
    # overlap, in bytes of the source's storage
    plane, frame = 640 * 480 * 4, 160 * 120 * 3 * 4
    for dst in (fake + plane - 4, fake - frame + 4):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + plane // 2 - 2, kind=F16)
    fails(b'src and dst overlap', dst=fake - frame // 2 + 2, dst_dtype=F16)
    fails(b'src and dst overlap', 'tdk_decode12_demosaic_scaled', dst=fake + 640 * 480 * 3 // 2 - 1)
    fails(b'gains and dst overlap', 'tdk_decode12_demosaic_scaled', dst=fake + 640 * 480 * 3 // 2, gains=fake + 640 * 480 * 3 // 2 + 8)
    # odd sizes are legal for the float forms, every legal ratio and a null gains pointer pass every check -- and would reach the launch: not made here


def test_host_queries(td):
    from torch_darktable._native import lib

    for sizes in ((640, 480, 160, 120), (2, 2, 1, 1), (3, 3, 1, 1), (7, 5, 3, 2), (65535, 65535, 4096, 4096), (64, 32, 4, 2)):
        assert lib.tdk_demosaic_scaled_lds_bytes(*sizes) == spec.LDS_BYTES <= 80 * 1024, sizes
        tw, th = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.tdk_demosaic_scaled_tile(*sizes, ctypes.byref(tw), ctypes.byref(th)) == 0
        assert (tw.value, th.value) == spec.tile(*sizes), sizes
    for bad in ((1, 2, 1, 1), (640, 480, 321, 120), (640, 480, 160, 29), (640, 480, 0, 120), (65536, 480, 4096, 120), (640, 480, 160, -1)):
        assert lib.tdk_demosaic_scaled_lds_bytes(*bad) == 0, bad
        tw, th = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.tdk_demosaic_scaled_tile(*bad, ctypes.byref(tw), ctypes.byref(th)) == INVALID_ARGUMENT and b'not a legal call' in lib.tdk_last_error()
    assert lib.tdk_demosaic_scaled_tile(640, 480, 160, 120, None, None) == INVALID_ARGUMENT and b'null pointer' in lib.tdk_last_error()
    # the staged row holds the widest footprint of either tile width, the intermediate the rows under the tile, the tables its taps
    for w, ow in ((4096, 2048), (4096, 512), (4097, 512), (65535, 4096), (33, 16), (64, 4)):
        tw, th = spec.tile(w, w, ow, ow)
        taps = (2 * w + ow - 1) // ow
        span = lambda t: ((t - 1) * w + 2 * w) // ow + 1
        assert 4 * span(tw) + 24 <= 136 * 16 and taps * tw <= 1024 and taps * th <= 512 and 2 * tw * span(th) <= 8192, (w, ow)
        xt = spec.axis_taps(w, ow) if w <= 4097 else None
        if xt is not None:   # the footprint of a tile, counted from the taps themselves
            for t0 in range(0, ow, tw):
                t1 = min(t0 + tw, ow) - 1
                assert xt[t1][0][-1] + 1 - xt[t0][0][0] <= span(tw) and max(len(j) for j, _ in xt[t0: t1 + 1]) <= taps


def test_package_exports_the_stage(td):
    import torch_darktable

    assert torch_darktable.ScaledDemosaic is torch_darktable.scaled_demosaic.ScaledDemosaic
    assert 'ScaledDemosaic' in torch_darktable.__all__ and 'scaled_demosaic' in torch_darktable.__all__
    assert torch_darktable.scaled_demosaic.__all__ == ['ScaledDemosaic']
    S = torch_darktable.ScaledDemosaic
    for name in ('process', 'process_packed', 'lds_bytes', 'longest_edge'):
        assert callable(getattr(S, name)), name
    for name in ('image_size', 'output_size', 'tile'):
        assert isinstance(getattr(S, name), property), name
    assert list(inspect.signature(S.__init__).parameters) == ['self', 'device', 'image_size', 'bayer_pattern', 'output_size']
    assert list(inspect.signature(S.longest_edge).parameters) == ['device', 'image_size', 'bayer_pattern', 'longest']
    params = inspect.signature(S.process).parameters
    assert list(params) == ['self', 'mosaic', 'white_balance', 'out_dtype'] and params['white_balance'].default is None and params['out_dtype'].default is None
    params = inspect.signature(S.process_packed).parameters
    assert list(params) == ['self', 'payload', 'packed_format', 'white_balance', 'out_dtype'] and params['white_balance'].default is None


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    S, P = td.ScaledDemosaic, td.BayerPattern.RGGB
    with pytest.raises(ValueError, match='CUDA'):
        S(torch.device('cpu'), (64, 48), P, (32, 24))
    for size in ((1, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='Image dimensions must be 2'):
            S(cuda, size, P, (32, 24))
    with pytest.raises(ValueError, match='Invalid bayer pattern'):
        S(cuda, (64, 48), 'RGGB', (32, 24))
    for out in ((0, 24), (32, -1)):
        with pytest.raises(ValueError, match='at least 1x1'):
            S(cuda, (64, 48), P, out)
    for out in ((33, 24), (32, 25), (64, 48)):
        with pytest.raises(ValueError, match='below 2:1'):
            S(cuda, (64, 48), P, out)
    for out in ((3, 24), (32, 2)):
        with pytest.raises(ValueError, match='beyond 16:1'):
            S(cuda, (64, 48), P, out)
    s = S(cuda, (64, 48), td.BayerPattern.GBRG, (21, 9))
    assert (s.width, s.height, s.image_size, s.out_width, s.out_height, s.output_size, s.bayer_pattern) == (64, 48, (64, 48), 21, 9, (21, 9), td.BayerPattern.GBRG)
    assert repr(s) == 'ScaledDemosaic(64x48 -> 21x9, GBRG)' and s.lds_bytes() == spec.LDS_BYTES and s.tile == spec.tile(64, 48, 21, 9)
    assert S(cuda, (7, 5), P, (3, 2)).output_size == (3, 2)   # odd mosaics are legal
    assert S.longest_edge(cuda, (4096, 3072), P, 1024).output_size == (1024, 768) and S.longest_edge(cuda, (3072, 4096), P, 512).output_size == (384, 512)
    with pytest.raises(ValueError, match='below 2:1'):
        S.longest_edge(cuda, (4096, 3072), P, 0)   # (0: the same size)
    with pytest.raises(AssertionError, match='2 dimensions'):
        s.process(torch.zeros(48, 64, 3))
    with pytest.raises(RuntimeError, match='expected'):
        s.process(torch.zeros(48, 32))
    with pytest.raises(RuntimeError, match='CUDA'):
        s.process(torch.zeros(48, 64))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        s.process(torch.zeros(48, 64, 1))
    with pytest.raises(RuntimeError, match='CUDA'):
        s.process_packed(torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match='Unsupported packed format'):
        s.process_packed(torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8), 'Packed12')
    with pytest.raises(ValueError, match='even width'):
        S(cuda, (7, 6), P, (3, 2)).process_packed(torch.zeros(63, dtype=torch.uint8))


def test_pipeline_takes_the_stage_as_a_property_only(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.camera_settings import CameraSettings

    assert not any('preview' in name for name in inspect.signature(ImageProcessor.__init__).parameters)
    assert list(inspect.signature(ImageProcessor.__init__).parameters)[-1] == 'raw_correction'
    for model in (ImageProcessingSettings, CameraSettings):
        assert not any('preview' in name for name in model.model_fields), model
    # a slot through _stage_property, wrapped: no stage of the chain `process` runs, so the chain's table of stages does not list it
    slot = vars(ImageProcessor)['preview']
    assert isinstance(slot._slot, property) and slot._slot.fset is not None and hasattr(type(slot), '__set__') and 'preview_processor' in slot.__doc__
    import pipeline_stack
    assert 'preview' not in pipeline_stack.stage_names_of(ImageProcessor)[1]
    assert isinstance(ImageProcessor.preview_processor, property) and ImageProcessor.preview_processor.fset is None
    assert ImageProcessor._preview is None and ImageProcessor._preview_processor is None   # the class-level defaults
    for name in ('process_preview', 'process_image_set_preview'):
        assert callable(getattr(ImageProcessor, name))
    assert 'PostProcess is not run' in ImageProcessor.process_preview.__doc__
    cuda = torch.device('cuda', 0)
    p = ImageProcessor.__new__(ImageProcessor)
    p.image_size, p.bayer_pattern = (64, 48), td.BayerPattern.RGGB
    assert '_preview' not in vars(p) and p.preview is None and p.preview_processor is None
    for bad in (object(), 3, 'preview', td.Resize(cuda, (64, 48), (32, 24))):
        with pytest.raises(TypeError, match='preview must be a ScaledDemosaic or None'):
            p.preview = bad
    for size in ((32, 48), (64, 50), (48, 64)):
        with pytest.raises(ValueError, match=rf'preview is for {size[0]}x{size[1]}, the processor for 64x48'):
            p.preview = td.ScaledDemosaic(cuda, size, td.BayerPattern.RGGB, (16, 16))
    with pytest.raises(ValueError, match='preview is for BGGR, the processor for RGGB'):
        p.preview = td.ScaledDemosaic(cuda, (64, 48), td.BayerPattern.BGGR, (32, 24))
    assert p.preview is None and p.preview_processor is None
    with pytest.raises(ValueError, match='process_preview needs preview'):
        p.process_image_set_preview({})
    p.preview = None
    assert p.preview is None
    source = inspect.getsource(ImageProcessor._load_preview)
    assert source.index('self.temporal.process') < source.index('self.chromatic.correct') < source.index('self.highlights.process') < source.index('preview.process(')
