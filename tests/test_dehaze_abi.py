"""CPU-only: the header include/tdk_hip_dehaze.h (haze removal) -- it parses to exactly its five declarations (exports and the
ctypes table: tests/test_header_abi.py), its constants and formulas are the ones the restatement uses, its source is part of the
build's source hash, every argument error of tdk_dehaze and tdk_dehaze_ambient is reported on the host before any HIP call, and the
Python front-end torch_darktable.Dehaze and the pipeline property raise the error types of the other operators."""

import ctypes
import inspect
import re
from pathlib import Path

import pytest

import dehaze_spec as spec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_dehaze.h'
EXPECTED = ['tdk_dehaze', 'tdk_dehaze_abi_version', 'tdk_dehaze_ambient', 'tdk_dehaze_lds_bytes', 'tdk_dehaze_workspace_bytes']
F32, F16, U8 = 0, 1, 2


def test_header_declares_the_haze_removal_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for name, value in (('ABI_VERSION', 1), ('MAX_DARK_RADIUS', 4), ('MAX_RADIUS', 8), ('MAX_CELLS', 16777216), ('PLANES', 10)):
        assert re.search(rf'#define TDK_DEHAZE_{name} {value}\b', text), name
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_dehaze'] == ('int', ['const void* src', 'void* dst', 'float* transmission_out', 'void* workspace', 'float* ambient', 'int width', 'int height',
                                           'int dtype', 'int cell', 'int dark_radius', 'int radius', 'int count', 'float eps', 'float strength', 'float floor',
                                           'const float* weights', 'int flags', 'tdk_stream_t stream'])
    assert decls['tdk_dehaze_ambient'] == ('int', ['const void* src', 'float* ambient', 'void* workspace', 'int width', 'int height', 'int dtype', 'int cell',
                                                   'int dark_radius', 'int count', 'int flags', 'tdk_stream_t stream'])
    assert decls['tdk_dehaze_workspace_bytes'] == ('size_t', ['int width', 'int height', 'int cell'])
    assert decls['tdk_dehaze_lds_bytes'] == ('size_t', ['int dtype', 'int cell', 'int dark_radius', 'int radius'])
    assert decls['tdk_dehaze_abi_version'] == ('int', [])
    for formula in ('pos(v) = v > 0 ? v : +0', 'm_c = minimum of pos(x_c) over the samples', 'M_c = tree(pos(x_c)) * (1 / (s*s))', 'Y = pos((w0*r + w1*g) + w2*b)',
                    'L = tree(Y) * (1 / (s*s))', 'd = minwin_rd(min(min(m0, m1), m2))', 'T = the K-th largest of the CW*CH values bits(d), counted with multiplicity',
                    'S = every cell with bits(d) >= T', 'fix(v) = (int64)(fminf(v, 65536) * 1048576)', 'ambient[c] = (float)(((double)sum_c / (double)n) * 2^-20)',
                    'ambient[3] = (float)n', 'A_c = fmaxf(ambient[c], 2^-10)', 'i_c = 1 / A_c', 'q = fminf(fminf(m0*i0, m1*i1), m2*i2)',
                    't = 1 - strength * fminf(minwin_rd(q), 1)', 'mL = box(L)*inv', 'mt = box(t)*inv', 'cov = box(L*t)*inv - mL*mt', 'var = pos(box(L*L)*inv - mL*mL)',
                    'a = cov / (var + eps)', 'b = mt - a*mL', 'A2 = box(a)*inv', 'B2 = box(b)*inv', 'q  = max(2*x + 1 - s, 0)', 'x0 = q / (2*s)',
                    'fx = (float)(q % (2*s)) / (2*s)', 'x1 = min(x0 + 1, CW - 1)', 'lerp(p0, p1, f) = p0 + f*(p1 - p0)', 'tp = fminf(fmaxf(Au*Y + Bu, floor), 1)',
                    'rt = 1 / tp', 'out_c = pos((x_c - A_c)*rt + A_c)', 'inv = (float)(1.0 / ((2rg+1)*(2rg+1)))'):
        assert formula in text, formula
    assert (_native.TDK_DEHAZE_MAX_DARK_RADIUS, _native.TDK_DEHAZE_MAX_RADIUS, _native.TDK_DEHAZE_MAX_CELLS, _native.TDK_DEHAZE_PLANES) == (4, 8, 1 << 24, 10)
    assert (spec.MAX_DARK_RADIUS, spec.MAX_RADIUS, spec.MAX_CELLS, spec.PLANES) == (4, 8, 1 << 24, 10) and float(spec.MIN_AMBIENT) == 2.0 ** -10
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_dehaze.h']
    assert rows == [('tdk_hip_dehaze.h', _native.DEHAZE_SIGNATURES, 'tdk_dehaze_abi_version', 1, 'dehaze ABI')]
    assert _native.ABI_VERSIONS['tdk_dehaze_abi_version'] == (1, 'dehaze ABI')
    assert sorted(_native.DEHAZE_SIGNATURES) == EXPECTED and _native.lib.tdk_dehaze_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'dehaze.hip') in build._inputs()
    assert [h.name for h in build.HEADERS] == [row[0] for row in _native.HEADERS]


def test_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    rec709 = (ctypes.c_float * 3)(0.2126, 0.7152, 0.0722)
    names = ['src', 'dst', 't', 'ws', 'amb', 'w', 'h', 'dtype', 'cell', 'rd', 'rg', 'count', 'eps', 'strength', 'floor', 'weights', 'flags', 'stream']
    args = [fake, fake + (1 << 24), fake + (2 << 24), fake + (3 << 24), fake + (4 << 24), 640, 480, F32, 8, 1, 4, 48, 1e-3, 0.9, 0.1, rec709, 0, None]
    est_names = ['src', 'amb', 'ws', 'w', 'h', 'dtype', 'cell', 'rd', 'count', 'flags', 'stream']
    est_args = [fake, fake + (4 << 24), fake + (3 << 24), 640, 480, F32, 8, 1, 48, 0, None]

    def fails(needle, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        assert lib.tdk_dehaze(*a) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())
        assert b'tdk_dehaze:' in lib.tdk_last_error()

    def estimate_fails(needle, **change):
        a = list(est_args)
        for k, v in change.items():
            a[est_names.index(k)] = v
        assert lib.tdk_dehaze_ambient(*a) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())
        assert b'tdk_dehaze_ambient:' in lib.tdk_last_error()

    for k in ('src', 'ws', 'amb', 'weights'):
        fails(b'null pointer', **{k: None})
    fails(b'null pointer (dst and transmission_out', dst=None, t=None)
    for k in ('w', 'h'):
        for v in (0, -2, 65536):
            fails(b'frame size', **{k: v})
    fails(b'cells is larger than 16777216', w=65535, h=65535, cell=2)
    fails(b'cells is larger than 16777216', w=65535, h=32770, cell=8)
    for d in (U8, 3, -1):
        fails(b'dtype', dtype=d)
    for c in (0, 1, 3, 5, 12, 32, -8):
        fails(b'cell must be 2, 4, 8 or 16', cell=c)
    for r in (-1, 5, 64):
        fails(b'dark_radius must be 0..4', rd=r)
    for r in (-1, 9, 64):
        fails(b': radius must be 0..8', rg=r)
    for c in (-1, 4801, 1 << 30):
        fails(b'count must be 0..4800', count=c)
    for e in (0.0, -1e-4, float('nan'), float('inf'), 1e-50):   # (1e-50 is 0 as a float32)
        fails(b'eps must be finite and > 0', eps=e)
    for s in (-0.01, 1.01, float('nan'), float('inf')):
        fails(b'strength must be in 0..1', strength=s)
    for f in (0.0, 0.0156, 1.001, float('nan'), -0.5):
        fails(b'floor must be in 2^-6..1', floor=f)
    for k, bad in enumerate((float('nan'), float('inf'), -0.5)):
        w = [0.2126, 0.7152, 0.0722]
        w[k] = bad
        fails(f'weights[{k}]'.encode(), weights=(ctypes.c_float * 3)(*w))
    for f in (1, 2, -1):
        fails(b'flags is reserved', flags=f)
    fails(b'ambient must be aligned', amb=fake + (4 << 24) + 2)
    fails(b'transmission_out must be aligned', t=fake + (2 << 24) + 1)
    # overlap, in bytes of the dtype
    frame, plane = 640 * 480 * 3 * 4, 640 * 480 * 4
    for dst in (fake, fake + 64, fake - frame + 4, fake + frame - 4):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + frame // 2 - 2, dtype=F16)
    for t in (fake + 128, fake + (1 << 24) - plane + 4, fake + (1 << 24) + frame - 4):
        fails(b'transmission_out overlaps src or dst', t=t)
    for amb in (fake + 16, fake + frame - 4, fake + (1 << 24) + 16, fake + (2 << 24) - 8):
        fails(b'ambient overlaps src, dst or transmission_out', amb=amb)
    fails(b'ambient overlaps', amb=fake + (2 << 24) - 8, dst=None, count=0)
    for ws in (fake + 16, fake + (1 << 24) - 64, fake + (2 << 24) + 4, fake + (4 << 24) - 100):
        fails(b'the workspace overlaps', ws=ws)
    # a dst just behind src, a transmission-only call, a frame-only call and count 0 pass every check -- and would reach the launch: not made here

    for k in ('src', 'ws', 'amb'):
        estimate_fails(b'null pointer', **{k: None})
    for k in ('w', 'h'):
        for v in (0, 65536):
            estimate_fails(b'frame size', **{k: v})
    estimate_fails(b'cells is larger than', w=65535, h=65535, cell=4)
    for d in (U8, -1):
        estimate_fails(b'dtype', dtype=d)
    for c in (0, 3, 32):
        estimate_fails(b'cell must be 2, 4, 8 or 16', cell=c)
    for r in (-1, 5):
        estimate_fails(b'dark_radius must be 0..4', rd=r)
    for c in (0, -1, 4801):
        estimate_fails(b'count must be 1..4800', count=c)
    estimate_fails(b'flags is reserved', flags=1)
    estimate_fails(b'ambient must be aligned', amb=fake + (4 << 24) + 3)
    for amb in (fake, fake + frame - 4):
        estimate_fails(b'ambient overlaps src', amb=amb)
    for ws in (fake + 16, fake + (4 << 24) - 100, fake + (4 << 24) + 8):
        estimate_fails(b'the workspace overlaps src or ambient', ws=ws)


def test_workspace_and_lds_queries(td):
    from torch_darktable._native import lib

    for (w, h, cell), cells in (((640, 480, 8), 80 * 60), ((641, 481, 8), 81 * 61), ((1, 1, 16), 1), ((5, 3, 2), 3 * 2), ((65535, 65535, 16), 4096 * 4096)):
        assert lib.tdk_dehaze_workspace_bytes(w, h, cell) == 10 * cells * 4 + 16, (w, h, cell)   # ten float32 planes
    for bad in ((0, 480, 8), (640, 65536, 8), (640, 480, 1), (640, 480, 3), (640, 480, 32), (65535, 65535, 8)):
        assert lib.tdk_dehaze_workspace_bytes(*bad) == 0, bad
    for tag in (F32, F16):
        sizes = [lib.tdk_dehaze_lds_bytes(tag, cell, 1, 4) for cell in (2, 4, 8, 16)]
        assert all(0 < s <= 65536 for s in sizes) and sizes == sorted(sizes, reverse=True), sizes
    for bad in ((U8, 8, 1, 4), (-1, 8, 1, 4), (F32, 1, 1, 4), (F32, 6, 1, 4), (F32, 8, -1, 4), (F32, 8, 5, 4), (F32, 8, 1, -1), (F32, 8, 1, 9)):
        assert lib.tdk_dehaze_lds_bytes(*bad) == 0, bad


def test_package_exports_the_haze_removal(td):
    import torch_darktable

    assert torch_darktable.Dehaze is torch_darktable.dehaze.Dehaze
    assert 'Dehaze' in torch_darktable.__all__ and 'dehaze' in torch_darktable.__all__
    assert torch_darktable.dehaze.__all__ == ['Dehaze']
    D = torch_darktable.Dehaze
    for name in ('process', 'transmission', 'estimate_ambient', 'set_ambient', 'workspace_bytes', 'lds_bytes'):
        assert callable(getattr(D, name)), name
    for name in ('ambient', 'image_size'):
        assert isinstance(getattr(D, name), property), name
    params = inspect.signature(D.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'strength', 'floor', 'cell', 'dark_radius', 'radius', 'eps', 'quantile', 'weights']
    assert [params[k].default for k in list(params)[3:]] == [0.9, 0.1, 8, 1, 4, 1e-3, 0.01, None]
    params = inspect.signature(D.process).parameters
    assert list(params) == ['self', 'image', 'ambient', 'return_transmission'] and params['ambient'].default is None and params['return_transmission'].default is False
    params = inspect.signature(D.transmission).parameters
    assert list(params) == ['self', 'image', 'ambient'] and params['ambient'].default is None
    assert list(inspect.signature(D.estimate_ambient).parameters) == ['self', 'image']
    assert list(inspect.signature(D.set_ambient).parameters) == ['self', 'ambient']
    assert list(inspect.signature(D.lds_bytes).parameters) == ['self', 'dtype'] and list(inspect.signature(D.workspace_bytes).parameters) == ['self']
    assert D.TILE == (128, 32)


def test_pipeline_takes_the_stage_as_a_property_only(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.camera_settings import CameraSettings

    assert not any('dehaze' in name or 'haze' in name for name in inspect.signature(ImageProcessor.__init__).parameters)
    assert not any('haze' in name for name in inspect.signature(ImageProcessor.from_camera_settings).parameters)
    assert list(inspect.signature(ImageProcessor.__init__).parameters)[-1] == 'raw_correction'
    for model in (ImageProcessingSettings, CameraSettings):
        assert not any('haze' in name for name in model.model_fields), model
    assert isinstance(ImageProcessor.dehaze, property) and ImageProcessor.dehaze.fset is not None
    assert ImageProcessor._dehaze is None   # the class-level default
    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    # an object made without the constructor has the slot through the class: the property needs the size only
    p = ImageProcessor.__new__(ImageProcessor)
    p.image_size = (64, 48)
    assert '_dehaze' not in vars(p) and p.dehaze is None
    for bad in (object(), 3, 'dh', td.ToneEqualizer(cuda, (64, 48))):
        with pytest.raises(TypeError, match='dehaze must be a Dehaze or None'):
            p.dehaze = bad
    for size in ((32, 48), (64, 50), (48, 64)):
        with pytest.raises(ValueError, match=rf'dehaze is for {size[0]}x{size[1]}, the processor for 64x48'):
            p.dehaze = td.Dehaze(cuda, size)
    assert p.dehaze is None
    dh = td.Dehaze(cuda, (64, 48))
    p.dehaze = dh
    assert p.dehaze is dh and ImageProcessor._dehaze is None
    p.dehaze = None
    assert p.dehaze is None
    source = inspect.getsource(ImageProcessor._process_frames)
    assert source.index('self.color.process') < source.index('self._dehaze.process') < source.index('self._tone_equalizer.process')


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)
    D = td.Dehaze
    with pytest.raises(ValueError, match='CUDA'):
        D(torch.device('cpu'), (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions must be 1'):
            D(cuda, size)
    with pytest.raises(ValueError, match='cells is larger than'):
        D(cuda, (65535, 65535), cell=8)
    for cell in (0, 1, 3, 32):
        with pytest.raises(ValueError, match='cell must be one of'):
            D(cuda, (64, 48), cell=cell)
    for radius in (-1, 5, 1.5):
        with pytest.raises(ValueError, match='dark_radius must be'):
            D(cuda, (64, 48), dark_radius=radius)
    for radius in (-1, 9, 2.5):
        with pytest.raises(ValueError, match='^radius must be'):
            D(cuda, (64, 48), radius=radius)
    for eps in (0.0, -1.0, float('nan'), float('inf'), 1e-50):
        with pytest.raises(ValueError, match='eps must be'):
            D(cuda, (64, 48), eps=eps)
    for strength in (-0.1, 1.1, float('nan')):
        with pytest.raises(ValueError, match='strength must be'):
            D(cuda, (64, 48), strength=strength)
    for floor in (0.0, 0.01, 1.5, float('nan')):
        with pytest.raises(ValueError, match='floor must be'):
            D(cuda, (64, 48), floor=floor)
    for quantile in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='quantile must be'):
            D(cuda, (64, 48), quantile=quantile)
    for weights in ((1, 1), (1, 1, -1), (1, float('nan'), 1)):
        with pytest.raises(ValueError, match='weights must be'):
            D(cuda, (64, 48), weights=weights)

    dh = D(cuda, (64, 48), strength=0.8, floor=0.25, cell=4, dark_radius=2, radius=3, eps=1e-2, quantile=0.1)
    assert (dh.width, dh.height, dh.image_size, dh.cell, dh.dark_radius, dh.radius, dh.floor, dh.quantile) == (64, 48, (64, 48), 4, 2, 3, 0.25, 0.1)
    assert dh.strength == ctypes.c_float(0.8).value and dh.eps == ctypes.c_float(1e-2).value
    assert dh.cells == 16 * 12 and dh.count == 19 == spec.count_of(0.1, 64, 48, 4)
    assert D(cuda, (7, 5)).count == 1 and D(cuda, (64, 48), quantile=1.0).count == 8 * 6
    assert dh.weights == tuple(ctypes.c_float(v).value for v in (0.2126, 0.7152, 0.0722))
    assert repr(dh) == 'Dehaze(64x48, strength=0.8, floor=0.25, cell=4, dark_radius=2, radius=3, eps=0.01, quantile=0.1)'
    assert dh.workspace_bytes() == 10 * 16 * 12 * 4 + 16
    assert 0 < dh.lds_bytes(torch.float16) <= 65536 and dh.lds_bytes(torch.float32) == dh.lds_bytes(torch.float16) and dh.lds_bytes(torch.uint8) == 0
    assert dh.ambient_is_fixed is False
    for bad in ((1, 2), (1, 2, float('nan')), torch.zeros(5), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match='ambient must be'):
            dh.set_ambient(bad)
    assert dh.ambient_is_fixed is False   # a refused set leaves the object as it was
    dh.set_ambient((0.8, 0.85, 0.9))
    assert dh.ambient_is_fixed is True
    dh.set_ambient(None)
    assert dh.ambient_is_fixed is False

    with pytest.raises(AssertionError, match='3 dimensions'):
        dh.process(torch.zeros(48, 64))
    with pytest.raises(RuntimeError, match='expected'):
        dh.process(torch.zeros(48, 32, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        dh.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        dh.transmission(torch.zeros(48, 64, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        dh.estimate_ambient(torch.zeros(48, 64, 3))
