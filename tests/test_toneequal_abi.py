"""CPU-only: the header include/tdk_hip_toneeq.h (tone equalizer) -- it parses to exactly its four declarations (exports and the
ctypes table: tests/test_header_abi.py), its constants and formulas are the ones the restatement uses, its source is part of the
build's source hash, every argument error of tdk_toneeq is reported on the host before any HIP call, and the Python front-end
torch_darktable.ToneEqualizer and the pipeline property raise the error types of the other operators."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import toneequal_spec as spec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_toneeq.h'
EXPECTED = ['tdk_toneeq', 'tdk_toneeq_abi_version', 'tdk_toneeq_lds_bytes', 'tdk_toneeq_workspace_bytes']
F32, F16, U8 = 0, 1, 2
GAINS = (3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0)


def test_header_declares_the_tone_equalizer_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for name, value in (('ABI_VERSION', 1), ('EV_MIN', -16), ('EV_MAX', 4), ('STEPS', 32), ('TABLE', 641), ('MAX_RADIUS', 8)):
        assert re.search(rf'#define TDK_TONEEQ_{name} {value}\b', text), name
    assert (4 + 16) * 32 + 1 == 641
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_toneeq'] == ('int', ['const void* src', 'void* dst', 'float* mask_out', 'void* workspace', 'const float* table', 'int width', 'int height',
                                           'int dtype', 'int cell', 'int radius', 'float eps', 'const float* weights', 'int flags', 'tdk_stream_t stream'])
    assert decls['tdk_toneeq_workspace_bytes'] == ('size_t', ['int width', 'int height', 'int cell'])
    assert decls['tdk_toneeq_lds_bytes'] == ('size_t', ['int dtype', 'int cell', 'int radius'])
    assert decls['tdk_toneeq_abi_version'] == ('int', [])
    for formula in ('Y = pos((w0*r + w1*g) + w2*b)', 'L = tree * (1 / (s*s))', 'mean = box(L)*inv', 'corr = box(L*L)*inv', 'var  = pos(corr - mean*mean)',
                    'a    = var / (var + eps)', 'b    = mean - a*mean', 'A = box(a)*inv', 'B = box(b)*inv', 'q  = max(2*x + 1 - s, 0)', 'x0 = q / (2*s)',
                    'fx = (float)(q % (2*s)) / (2*s)', 'x1 = min(x0 + 1, CW - 1)', 'lerp(p0, p1, f) = p0 + f*(p1 - p0)', 'm  = Au*Y + Bu',
                    'mc = fminf(fmaxf(m, 2^-16), 16 - 2^-20)', 'i  = (e + 16)*32 + (M >> 18)', 'f = (float)(M & 0x3FFFF) / 262144', 'gain = T[i] + f*(T[i+1] - T[i])',
                    'out[c] = x[c] * gain', 'inv = (float)(1.0 / ((2r+1)*(2r+1)))'):
        assert formula in text, formula
    assert (_native.TDK_TONEEQ_EV_MIN, _native.TDK_TONEEQ_EV_MAX, _native.TDK_TONEEQ_STEPS, _native.TDK_TONEEQ_TABLE, _native.TDK_TONEEQ_MAX_RADIUS) == (-16, 4, 32, 641, 8)
    assert (spec.EV_MIN, spec.EV_MAX, spec.STEPS, spec.TABLE) == (-16, 4, 32, 641) and float(spec.M_HI) == 16 - 2.0 ** -20
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_toneeq.h']
    assert rows == [('tdk_hip_toneeq.h', _native.TONEEQ_SIGNATURES, 'tdk_toneeq_abi_version', 1, 'tone equalizer ABI')]
    assert _native.ABI_VERSIONS['tdk_toneeq_abi_version'] == (1, 'tone equalizer ABI')
    assert sorted(_native.TONEEQ_SIGNATURES) == EXPECTED and _native.lib.tdk_toneeq_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'toneequal.hip') in build._inputs()


def test_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    rec709 = (ctypes.c_float * 3)(0.2126, 0.7152, 0.0722)
    names = ['src', 'dst', 'mask', 'ws', 'table', 'w', 'h', 'dtype', 'cell', 'radius', 'eps', 'weights', 'flags', 'stream']
    args = [fake, fake + (1 << 24), fake + (2 << 24), fake + (3 << 24), fake + (4 << 24), 640, 480, F32, 8, 4, 1e-4, rec709, 0, None]

    def fails(needle, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        assert lib.tdk_toneeq(*a) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())

    for k in ('src', 'ws', 'table', 'weights'):
        fails(b'null pointer', **{k: None})
    fails(b'null pointer (dst and mask_out', dst=None, mask=None)
    for k in ('w', 'h'):
        for v in (0, -2, 65536):
            fails(b'frame size', **{k: v})
    for d in (U8, 3, -1):
        fails(b'dtype', dtype=d)
    for c in (0, 1, 3, 5, 12, 32, -8):
        fails(b'cell must be 2, 4, 8 or 16', cell=c)
    for r in (-1, 9, 64):
        fails(b'radius must be 0..8', radius=r)
    for e in (0.0, -1e-4, float('nan'), float('inf'), 1e-50):   # (1e-50 is 0 as a float32)
        fails(b'eps must be finite and > 0', eps=e)
    for k, bad in enumerate((float('nan'), float('inf'), -0.5)):
        w = [0.2126, 0.7152, 0.0722]
        w[k] = bad
        fails(f'weights[{k}]'.encode(), weights=(ctypes.c_float * 3)(*w))
    for f in (1, 2, -1):
        fails(b'flags is reserved', flags=f)
    fails(b'table must be aligned', table=fake + (4 << 24) + 2)
    fails(b'mask_out must be aligned', mask=fake + (2 << 24) + 1)
    # overlap, in bytes of the dtype
    frame, plane = 640 * 480 * 3 * 4, 640 * 480 * 4
    for dst in (fake, fake + 64, fake - frame + 4, fake + frame - 4):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + frame // 2 - 2, dtype=F16)
    for mask in (fake + 128, fake + (1 << 24) - plane + 4, fake + (1 << 24) + frame - 4):
        fails(b'mask_out overlaps src or dst', mask=mask)
    fails(b'the table overlaps dst or mask_out', table=fake + (1 << 24) + 16)
    fails(b'the table overlaps dst or mask_out', table=fake + (2 << 24) - 8, dst=None)
    for ws in (fake + 16, fake + (1 << 24) - 64, fake + (2 << 24) + 4, fake + (4 << 24) - 100):
        fails(b'the workspace overlaps', ws=ws)
    assert b'tdk_toneeq:' in lib.tdk_last_error()
    # a dst just behind src, a mask-only call and a frame-only call pass every check -- and would reach the launch: not made here


def test_workspace_and_lds_queries(td):
    from torch_darktable._native import lib

    for (w, h, cell), cells in (((640, 480, 8), 80 * 60), ((641, 481, 8), 81 * 61), ((1, 1, 16), 1), ((5, 3, 2), 3 * 2), ((65535, 65535, 2), 32768 * 32768)):
        assert lib.tdk_toneeq_workspace_bytes(w, h, cell) == 3 * cells * 4 + 16, (w, h, cell)   # three float32 planes: L, a, b
    for bad in ((0, 480, 8), (640, 65536, 8), (640, 480, 1), (640, 480, 3), (640, 480, 32)):
        assert lib.tdk_toneeq_workspace_bytes(*bad) == 0, bad
    for tag in (F32, F16):
        sizes = [lib.tdk_toneeq_lds_bytes(tag, cell, 4) for cell in (2, 4, 8, 16)]
        assert all(0 < s <= 65536 for s in sizes) and sizes == sorted(sizes, reverse=True), sizes
    for bad in ((U8, 8, 4), (-1, 8, 4), (F32, 1, 4), (F32, 6, 4), (F32, 8, -1), (F32, 8, 9)):
        assert lib.tdk_toneeq_lds_bytes(*bad) == 0, bad


def test_package_exports_the_tone_equalizer(td):
    import torch_darktable

    assert torch_darktable.ToneEqualizer is torch_darktable.toneequal.ToneEqualizer
    assert 'ToneEqualizer' in torch_darktable.__all__ and 'toneequal' in torch_darktable.__all__
    assert torch_darktable.toneequal.__all__ == ['ToneEqualizer']
    T = torch_darktable.ToneEqualizer
    for name in ('process', 'mask', 'set_gains', 'workspace_bytes', 'lds_bytes', 'curve'):
        assert callable(getattr(T, name)), name
    for name in ('table', 'gains_ev'):
        assert isinstance(getattr(T, name), property), name
    params = inspect.signature(T.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'gains_ev', 'cell', 'radius', 'eps', 'mask_exposure', 'sigma', 'weights']
    assert [params[k].default for k in list(params)[3:]] == [(0,) * 9, 8, 4, 1e-4, 0.0, 2 ** 0.5, None]
    params = inspect.signature(T.process).parameters
    assert list(params) == ['self', 'image', 'return_mask'] and params['return_mask'].default is False
    assert list(inspect.signature(T.mask).parameters) == ['self', 'image']
    params = inspect.signature(T.set_gains).parameters
    assert list(params) == ['self', 'gains_ev', 'mask_exposure'] and params['mask_exposure'].default is None
    params = inspect.signature(T.curve).parameters
    assert list(params) == ['gains_ev', 'sigma'] and params['sigma'].default == 2 ** 0.5
    assert list(inspect.signature(T.lds_bytes).parameters) == ['self', 'dtype'] and list(inspect.signature(T.workspace_bytes).parameters) == ['self']
    assert T.TILE == (128, 32)


def test_host_curve_is_the_restatements(td):
    T = td.ToneEqualizer
    for gains, exposure, sigma in ((GAINS, 0.0, 2 ** 0.5), ((2, 2, 1.5, 1, 0.5, 0, 0, -0.5, -1), -1.5, 2 ** 0.5), ((0,) * 9, 2.0, 2 ** 0.5), (GAINS, 0.25, 1.2)):
        assert np.array_equal(T.curve(gains, sigma), spec.curve(gains, sigma))
        table = T.make_table(gains, exposure, sigma)
        assert table.dtype == np.float32 and table.shape == (641,)
        assert np.array_equal(table.view(np.uint32), spec.make_table(gains, exposure, sigma).view(np.uint32))
    assert np.array_equal(T.table_nodes(), spec.nodes())
    assert np.array_equal(T.make_table((0,) * 9), np.ones(641, dtype=np.float32))
    assert np.abs(T.correction(np.arange(-8.0, 1.0), T.curve(GAINS)) - np.asarray(GAINS)).max() < 1e-12


def test_pipeline_takes_the_stage_as_a_property_only(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.camera_settings import CameraSettings

    assert not any('tone_eq' in name or 'toneeq' in name for name in inspect.signature(ImageProcessor.__init__).parameters)
    assert not any('tone_eq' in name for name in inspect.signature(ImageProcessor.from_camera_settings).parameters)
    assert list(inspect.signature(ImageProcessor.__init__).parameters)[-1] == 'raw_correction'
    for model in (ImageProcessingSettings, CameraSettings):
        assert not any('tone_eq' in name or 'toneeq' in name for name in model.model_fields), model
    assert isinstance(ImageProcessor.tone_equalizer, property) and ImageProcessor.tone_equalizer.fset is not None
    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    # a processor's constructor puts its workspaces on the device; the property needs the size and its own slot only
    p = ImageProcessor.__new__(ImageProcessor)
    p.image_size, p._tone_equalizer = (64, 48), None
    assert p.tone_equalizer is None
    for bad in (object(), 3, 'te', td.Wavelet(cuda, (64, 48))):
        with pytest.raises(TypeError, match='tone_equalizer must be a ToneEqualizer or None'):
            p.tone_equalizer = bad
    for size in ((32, 48), (64, 50), (48, 64)):
        with pytest.raises(ValueError, match=rf'tone_equalizer is for {size[0]}x{size[1]}, the processor for 64x48'):
            p.tone_equalizer = td.ToneEqualizer(cuda, size)
    assert p.tone_equalizer is None
    te = td.ToneEqualizer(cuda, (64, 48), gains_ev=GAINS)
    p.tone_equalizer = te
    assert p.tone_equalizer is te
    p.tone_equalizer = None
    assert p.tone_equalizer is None


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)
    T = td.ToneEqualizer
    with pytest.raises(ValueError, match='CUDA'):
        T(torch.device('cpu'), (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions must be 1'):
            T(cuda, size)
    for cell in (0, 1, 3, 32):
        with pytest.raises(ValueError, match='cell must be one of'):
            T(cuda, (64, 48), cell=cell)
    for radius in (-1, 9, 2.5):
        with pytest.raises(ValueError, match='radius must be'):
            T(cuda, (64, 48), radius=radius)
    for eps in (0.0, -1.0, float('nan'), float('inf'), 1e-50):
        with pytest.raises(ValueError, match='eps must be'):
            T(cuda, (64, 48), eps=eps)
    for weights in ((1, 1), (1, 1, -1), (1, float('nan'), 1)):
        with pytest.raises(ValueError, match='weights must be'):
            T(cuda, (64, 48), weights=weights)
    with pytest.raises(ValueError, match='sigma must be'):
        T(cuda, (64, 48), sigma=0.0)
    with pytest.raises(ValueError, match='9 values'):
        T(cuda, (64, 48), gains_ev=(1, 2, 3))
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='must be finite'):
            T(cuda, (64, 48), gains_ev=(0, 0, 0, bad, 0, 0, 0, 0, 0))
    with pytest.raises(ValueError, match='mask_exposure must be finite'):
        T(cuda, (64, 48), mask_exposure=float('nan'))
    # the pole check: a curve that swings more than 1 EV outside its nodes between them
    with pytest.raises(ValueError, match='ill-conditioned'):
        T(cuda, (64, 48), gains_ev=(3, -3, 3, -3, 3, -3, 3, -3, 3))
    w = spec.curve((3, -3, 3, -3, 3, -3, 3, -3, 3))
    assert spec.correction(np.linspace(-8, 0, 129), w).min() < -3 - 1

    te = T(cuda, (64, 48), gains_ev=GAINS, cell=4, radius=2, eps=1e-3, mask_exposure=0.5)
    assert (te.width, te.height, te.image_size, te.cell, te.radius, te.mask_exposure, te.sigma) == (64, 48, (64, 48), 4, 2, 0.5, 2 ** 0.5)
    assert te.gains_ev == tuple(float(g) for g in GAINS) and te.eps == ctypes.c_float(1e-3).value
    assert te.weights == tuple(ctypes.c_float(v).value for v in (0.2126, 0.7152, 0.0722))
    assert repr(te) == 'ToneEqualizer(64x48, gains_ev=(3.0, 3.0, 3.0, 2.5, 2.0, 1.5, 1.0, 0.5, 0.0), cell=4, radius=2, eps=0.001, mask_exposure=0.5)'
    assert te.workspace_bytes() == 3 * 16 * 12 * 4 + 16
    assert 0 < te.lds_bytes(torch.float16) <= 65536 and te.lds_bytes(torch.float32) == te.lds_bytes(torch.float16) and te.lds_bytes(torch.uint8) == 0
    with pytest.raises(ValueError, match='ill-conditioned'):
        te.set_gains((3, -3, 3, -3, 3, -3, 3, -3, 3))
    assert te.gains_ev == tuple(float(g) for g in GAINS)   # a refused set leaves the object as it was
    te.set_gains((0,) * 9, mask_exposure=1.0)
    assert te.gains_ev == (0.0,) * 9 and te.mask_exposure == 1.0

    with pytest.raises(AssertionError, match='3 dimensions'):
        te.process(torch.zeros(48, 64))
    with pytest.raises(RuntimeError, match='expected'):
        te.process(torch.zeros(48, 32, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        te.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        te.mask(torch.zeros(48, 64, 3))
