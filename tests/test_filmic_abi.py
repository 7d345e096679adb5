"""CPU-only: the header include/tdk_hip_filmic.h (scene-referred tone mapping) -- it parses to exactly its three declarations (exports
and the ctypes table: tests/test_header_abi.py), its constants and formulas are the ones the restatement uses, its source is part of
the build's source hash, every argument error of tdk_filmic is reported on the host before any HIP call, and the Python front-end
torch_darktable.Filmic and the pipeline property raise the error types of the other operators."""

import ctypes
import inspect
import re
from pathlib import Path

import pytest

import filmic_spec as spec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_filmic.h'
EXPECTED = ['tdk_filmic', 'tdk_filmic_abi_version', 'tdk_filmic_lds_bytes']
F32, F16, U8 = 0, 1, 2


def test_header_declares_the_filmic_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for name, value in (('ABI_VERSION', 1), ('EV_MIN', -20), ('EV_MAX', 12), ('STEPS', 32), ('TABLE', 1025), ('ENC_EV_MIN', -16), ('ENC_TABLE', 513), ('MAX', 0), ('LUMA', 1),
                        ('POWER', 2), ('NONE', 3)):
        assert re.search(rf'#define TDK_FILMIC_{name} {value}\b', text), name
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_filmic'] == ('int', ['const void* src', 'void* dst', 'const float* curve', 'const float* encode', 'const float* exposure', 'int64_t npix',
                                           'int src_dtype', 'int dst_dtype', 'int norm', 'const float* weights', 'int flags', 'tdk_stream_t stream'])
    assert decls['tdk_filmic_lds_bytes'] == ('size_t', []) and decls['tdk_filmic_abi_version'] == ('int', [])
    for formula in ('pos(v) = v > 0 ? v : +0', 'p_c = fminf(pos(x_c * e), XMAX)', 'N = fmaxf(fmaxf(p0, p1), p2)', 'N = (w0*p0 + w1*p1) + w2*p2', 'q_c = p_c*p_c',
                    'k_c = q_c*p_c', 'den = (q0 + q1) + q2', 'num = (k0 + k1) + k2', 'N = den > 0 ? num / den : +0', 'Nc = fminf(fmaxf(N, XMIN), XMAX)',
                    'ex = (bits(Nc) >> 23) - 127', 'M = bits(Nc) & 0x7FFFFF', 'i  = (ex + 20)*32 + (M >> 18)', 'f = (float)(M & 0x3FFFF) / 262144',
                    'y  = T[i] + f*(T[i+1] - T[i])', 'd  = D[i] + f*(D[i+1] - D[i])', 'r_c = p_c / Nc', 's_c = 1 + d*(r_c - 1)', 'o_c = y * s_c',
                    'm = fmaxf(fmaxf(o0, o1), o2)', 'g = (1 - y) / (m - y)', 'o_c = y + (o_c - y)*g', 'oc = fminf(pos(o_c), 1 - 2^-24)', 'v_c = (oc * 65536) * G[0]',
                    'i  = (ex + 16)*32 + (M >> 18)', 'v_c = G[i] + f*(G[i+1] - G[i])', 'rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f)',
                    'node j stands at (1 + (j % 32) / 32) * 2^(j / 32 - 20)', '16 * (TDK_FILMIC_TABLE - 1) + 8 * (TDK_FILMIC_ENC_TABLE - 1) = 20480'):
        assert formula in text, formula
    assert (_native.TDK_FILMIC_EV_MIN, _native.TDK_FILMIC_EV_MAX, _native.TDK_FILMIC_STEPS, _native.TDK_FILMIC_TABLE) == (spec.EV_MIN, spec.EV_MAX, spec.STEPS, spec.TABLE)
    assert spec.TABLE == (spec.EV_MAX - spec.EV_MIN) * spec.STEPS + 1 and spec.ENC_TABLE == -spec.ENC_EV_MIN * spec.STEPS + 1
    rows = [row[0] for row in _native.HEADERS]
    assert _native.HEADERS[rows.index('tdk_hip_filmic.h')] == ('tdk_hip_filmic.h', _native.FILMIC_SIGNATURES, 'tdk_filmic_abi_version', 1, 'filmic ABI')
    assert rows.index('tdk_hip_filmic.h') == rows.index('tdk_hip_dehaze.h') + 1   # directly behind the haze removal
    assert rows[-3:] == ['tdk_hip_stats.h', 'tdk_hip_noise.h', 'tdk_hip_lut.h'] and rows.index('tdk_hip_rawcodec.h') == rows.index('tdk_hip_ca.h') + 1
    assert _native.ABI_VERSIONS['tdk_filmic_abi_version'] == (1, 'filmic ABI')
    assert sorted(_native.FILMIC_SIGNATURES) == EXPECTED and _native.lib.tdk_filmic_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'filmic.hip') in build._inputs()
    assert [h.name for h in build.HEADERS] == rows


def test_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    rec709 = (ctypes.c_float * 3)(0.2126, 0.7152, 0.0722)
    names = ['src', 'dst', 'curve', 'encode', 'exposure', 'npix', 'src_dtype', 'dst_dtype', 'norm', 'weights', 'flags', 'stream']
    args = [fake, fake + (1 << 24), fake + (2 << 24), fake + (3 << 24), fake + (4 << 24), 640 * 480, F32, U8, 0, rec709, 0, None]

    def fails(needle, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        assert lib.tdk_filmic(*a) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())
        assert b'tdk_filmic:' in lib.tdk_last_error()

    for k in ('src', 'dst', 'curve', 'exposure', 'weights'):
        fails(f'null pointer ({k})'.encode(), **{k: None})
    for n in (-1, -(1 << 40), 1 << 62):
        fails(b'npix', npix=n)
    for d in (U8, 3, -1):
        fails(b'source dtype', src_dtype=d)
    for d in (3, -1, 7):
        fails(b'destination dtype', dst_dtype=d)
    for n in (-1, 4, 100):
        fails(b'norm must be', norm=n)
    for k, bad in enumerate((float('nan'), float('inf'), -0.5)):
        w = [0.2126, 0.7152, 0.0722]
        w[k] = bad
        fails(f'weights[{k}]'.encode(), weights=(ctypes.c_float * 3)(*w))
    for f in (1, 2, -1):
        fails(b'flags is reserved', flags=f)
    for k in ('curve', 'encode', 'exposure'):
        for off in (1, 2, 3):
            fails(f'{k} must be aligned'.encode(), **{k: args[names.index(k)] + off})
    fails(b'src must be aligned', src=fake + 2)
    fails(b'src must be aligned', src=fake + 1, src_dtype=F16)
    fails(b'dst must be aligned', dst=fake + (1 << 24) + 2, dst_dtype=F32)
    fails(b'dst must be aligned', dst=fake + (1 << 24) + 1, dst_dtype=F16)
    # overlap, in bytes of the two types
    src_bytes, n = 640 * 480 * 3 * 4, 640 * 480 * 3
    for dst in (fake, fake + 64, fake - n + 1, fake + src_bytes - 1):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + src_bytes // 2 - 2, src_dtype=F16, dst_dtype=F16)
    fails(b'src and dst overlap', dst=fake - src_bytes + 4, dst_dtype=F32)
    for curve in (fake + (1 << 24), fake + (1 << 24) + n - 4, fake + (1 << 24) - 2 * 1025 * 4 + 4):
        fails(b'curve and dst overlap', curve=curve)
    for encode in (fake + (1 << 24) + 8, fake + (1 << 24) - 513 * 4 + 4):
        fails(b'encode and dst overlap', encode=encode)
    for exposure in (fake + (1 << 24), fake + (1 << 24) + n - 4):
        fails(b'exposure and dst overlap', exposure=exposure)
    # a dst just behind src, tables just in front of dst, a null encode and npix 0 pass every check; only the last returns without a launch
    a = list(args)
    a[names.index('npix')] = 0
    assert lib.tdk_filmic(*a) == 0
    a[names.index('encode')] = None
    assert lib.tdk_filmic(*a) == 0


def test_lds_query(td):
    from torch_darktable._native import lib

    assert lib.tdk_filmic_lds_bytes() == 16 * 1024 + 8 * 512 == 20480
    assert lib.tdk_filmic_lds_bytes() <= 64 * 1024


def test_package_exports_the_stage(td):
    import torch
    import torch_darktable

    assert torch_darktable.Filmic is torch_darktable.filmic.Filmic
    assert 'Filmic' in torch_darktable.__all__ and 'filmic' in torch_darktable.__all__
    assert torch_darktable.filmic.__all__ == ['Filmic']
    Fm = torch_darktable.Filmic
    for name in ('process', 'set_exposure', 'set_curve', 'sigmoid', 'from_curve', 'table_nodes'):
        assert callable(getattr(Fm, name)), name
    for name in ('exposure', 'curve_table', 'encode_table', 'lds_bytes'):
        assert isinstance(getattr(Fm, name), property), name
    params = inspect.signature(Fm.__init__).parameters
    assert list(params) == ['self', 'device', 'grey', 'black_ev', 'white_ev', 'contrast', 'latitude', 'target', 'output_power', 'desaturate', 'norm', 'encoding', 'weights']
    assert [params[k].default for k in list(params)[2:]] == [0.18, -8.0, None, 1.5, 0.25, (0.0, 0.1845, 1.0), None, (0.0, 1.0), 'max', 'srgb', None]
    params = inspect.signature(Fm.sigmoid).parameters
    assert list(params)[:4] == ['device', 'grey', 'contrast', 'target_grey'] and [params[k].default for k in ('grey', 'contrast', 'target_grey')] == [0.18, 1.5, 0.1845]
    assert list(inspect.signature(Fm.from_curve).parameters)[:3] == ['device', 'fn', 'desaturation']
    params = inspect.signature(Fm.process).parameters
    assert list(params) == ['self', 'image', 'out_dtype', 'out'] and params['out_dtype'].default is torch.uint8 and params['out'].default is None
    assert Fm.GROUP == 16


def test_pipeline_takes_the_stage_as_a_property_only(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.camera_settings import CameraSettings

    assert not any('filmic' in name for name in inspect.signature(ImageProcessor.__init__).parameters)
    assert not any('filmic' in name for name in inspect.signature(ImageProcessor.from_camera_settings).parameters)
    assert list(inspect.signature(ImageProcessor.__init__).parameters)[-1] == 'raw_correction'
    for model in (ImageProcessingSettings, CameraSettings):
        assert not any('filmic' in name for name in model.model_fields), model
    assert isinstance(ImageProcessor.filmic, property) and ImageProcessor.filmic.fset is not None
    assert ImageProcessor._filmic is None   # the class-level default
    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    p = ImageProcessor.__new__(ImageProcessor)   # an object made without the constructor has the slot through the class
    assert '_filmic' not in vars(p) and p.filmic is None
    for bad in (object(), 3, 'filmic', td.ColorLUT.identity(cuda, 2)):
        with pytest.raises(TypeError, match='filmic must be a Filmic or None'):
            p.filmic = bad
    assert p.filmic is None
    f = td.Filmic(cuda)
    p.filmic = f
    assert p.filmic is f and ImageProcessor._filmic is None
    p.filmic = None
    assert p.filmic is None
    source = inspect.getsource(ImageProcessor._process_frames)
    assert source.count('self.tonemap(img, self.metrics)') == 1 and source.index('self._filmic.process(img)') < source.index('self.tonemap(img, self.metrics)')
    assert source.index('acc.finish()') < source.index('self._filmic.process(img)') < source.index('self.look.process')   # metrics as before, the look behind it


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)
    Fm = td.Filmic
    for make in (Fm, Fm.sigmoid, lambda device, **kw: Fm.from_curve(device, lambda x: x, **kw)):
        with pytest.raises(ValueError, match='CUDA'):
            make(torch.device('cpu'))
        for norm in ('euclid', 'MAX', None, 0):
            with pytest.raises(ValueError, match='norm must be one of'):
                make(cuda, norm=norm)
        for weights in ((1, 1), (1, 1, -1), (1, float('nan'), 1)):
            with pytest.raises(ValueError, match='weights must be'):
                make(cuda, weights=weights)
        with pytest.raises(ValueError, match='encoding must be'):
            make(cuda, encoding='linear')
    for kw, message in ((dict(grey=-1.0), 'grey and contrast'), (dict(contrast=0.0), 'grey and contrast'), (dict(target_grey=1.0), 'target_grey must be'),
                        (dict(desaturate=2.0), 'desaturate must be'), (dict(desaturate_ev=(3.0, 1.0)), 'desaturate must be'), (dict(contrast=float('inf')), 'finite')):
        with pytest.raises(ValueError, match=message):
            Fm.sigmoid(cuda, **kw)

    f = Fm(cuda, norm='luma', weights=(0.25, 0.5, 0.25))
    assert (f.norm, f.encoding, f.weights, f.lds_bytes) == ('luma', 'srgb', (0.25, 0.5, 0.25), 20480)
    assert repr(f) == "Filmic(filmic, norm='luma', encoding='srgb', lds=20480)"
    assert repr(Fm.sigmoid(cuda, encoding=None)) == "Filmic(sigmoid, norm='max', encoding=None, lds=20480)"
    assert tuple(f.host_curve.shape) == (2, 1025) and tuple(f.host_encode.shape) == (513,) and f.host_curve.dtype == f.host_encode.dtype == torch.float32
    for bad in (float('nan'), float('inf'), -1.0, torch.zeros(2), torch.zeros(1, dtype=torch.float64)):
        with pytest.raises(ValueError, match='exposure must be'):
            f.set_exposure(bad)
    f.set_exposure(2.0)
    with pytest.raises(ValueError, match='not both'):
        f.set_curve(lambda x: x, contrast=1.0)
    with pytest.raises(ValueError, match='takes the spline parameters'):
        f.set_curve(gamma=2.0)
    with pytest.raises(ValueError, match='give set_curve a function'):
        Fm.sigmoid(cuda).set_curve(contrast=1.0)

    with pytest.raises(ValueError, match='three channels'):
        f.process(torch.zeros(48, 64))
    with pytest.raises(ValueError, match='float32 or float16'):
        f.process(torch.zeros(48, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='out_dtype must be'):
        f.process(torch.zeros(48, 64, 3), out_dtype=torch.int16)
    with pytest.raises(RuntimeError, match='CUDA'):
        f.process(torch.zeros(48, 64, 3))   # no CPU fallback
