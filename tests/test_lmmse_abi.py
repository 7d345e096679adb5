"""CPU-only: the header include/tdk_hip_lmmse.h (the demosaic for noisy frames) -- it parses to exactly its three declarations
(exports and the ctypes table: tests/test_header_abi.py), its constants and formulas are the ones the restatement uses, its source is
part of the build's source hash, every argument error of tdk_lmmse is reported on the host before any HIP call, and the Python
front-end torch_darktable.LMMSE and the pipeline property ImageProcessor.demosaic raise the error types of the other operators.  The
stand-alone program tests/hip_unit/lmmse_arguments_main.cpp makes the same calls for a run under a host sanitizer."""

import inspect
import re
from pathlib import Path

import pytest

import lmmse_spec as spec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_lmmse.h'
EXPECTED = ['tdk_lmmse', 'tdk_lmmse_abi_version', 'tdk_lmmse_lds_bytes']
F32, F16, U8 = 0, 1, 2
LINEAR = 1


def test_header_declares_the_lmmse_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for name, value in (('ABI_VERSION', 1), ('LINEAR', 1), ('TILE_W', 32), ('TILE_H', 32), ('APRON', 11), ('MIN_SIZE', 2), ('MAX_SIZE', 65535)):
        assert re.search(rf'#define TDK_LMMSE_{name} {value}\b', text), name
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_lmmse'] == ('int', ['const void* src', 'void* dst', 'int width', 'int height', 'uint32_t pattern', 'int src_dtype', 'int dst_dtype', 'int flags',
                                          'tdk_stream_t stream'])
    assert decls['tdk_lmmse_lds_bytes'] == ('size_t', ['int src_dtype', 'int dst_dtype', 'int flags'])
    assert decls['tdk_lmmse_abi_version'] == ('int', [])
    for formula in ('t = sqrtf(fmaxf(m, 0))', 't = m ', 'e = (0.5*(t[-1] + t[+1]) - 0.25*(t[-2] + t[+2])) + 0.5*t[0]', 'd = e - t[0]', 'd = t[0] - e',
                    'p = g0*d[0]', 'p = p + gk*(d[-k] + d[+k])', 'S(a) = a[0]', 'S = S + (a[-k] + a[+k])', 'mu = S(p) * NINTH', 'vx = EPS + S(a)',
                    'a[k] = (p[k] - mu)*(p[k] - mu)', 'vn = EPS + S(b)', 'b[k] = (d[k] - p[k])*(d[k] - p[k])', 'x  = (p[0]*vn + d[0]*vx) / (vx + vn)',
                    'v  = (vx*vn) / (vx + vn)', 'D = (x_h*v_v + x_v*v_h) / (v_h + v_v)', 'G = t + D', 'C = G - 0.5*(D[-1] + D[+1])',
                    'C = G - 0.25*((D[-1,-1] + D[-1,+1]) + (D[+1,-1] + D[+1,+1]))', 'q*q with q = fmaxf(c, 0)', '-k -> k, n-1+k -> n-1-k'):
        assert formula in text, formula
    # the literals the header prints are the restatement's values
    for k, value in enumerate(spec.G):
        assert re.search(rf'g{k} = {re.escape(float(value).hex().replace("0000000p", "p"))}f', text), (k, float(value).hex())
    assert 'NINTH = 0x1.c71c72p-4f' in text and float(spec.NINTH).hex() == '0x1.c71c720000000p-4'
    assert 'EPS = 1e-7f = 0x1.ad7f2ap-24f' in text and float(spec.EPS).hex() == '0x1.ad7f2a0000000p-24'
    assert (_native.TDK_LMMSE_LINEAR, _native.TDK_LMMSE_TILE_W, _native.TDK_LMMSE_TILE_H, _native.TDK_LMMSE_APRON) == (1, 32, 32, 11) == (spec.LINEAR, 32, 32, spec.APRON)
    assert (_native.TDK_LMMSE_MIN_SIZE, _native.TDK_LMMSE_MAX_SIZE) == (2, 65535)
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_lmmse.h']
    assert rows == [('tdk_hip_lmmse.h', _native.LMMSE_SIGNATURES, 'tdk_lmmse_abi_version', 1, 'LMMSE demosaic ABI')]
    assert _native.ABI_VERSIONS['tdk_lmmse_abi_version'] == (1, 'LMMSE demosaic ABI')
    assert sorted(_native.LMMSE_SIGNATURES) == EXPECTED and _native.lib.tdk_lmmse_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'lmmse.hip') in build._inputs()
    assert [h.name for h in build.HEADERS] == [row[0] for row in _native.HEADERS]
    # the pattern words of tdk_hip.h are the restatement's
    base = (ROOT / 'include' / 'tdk_hip.h').read_text()
    for name, word in spec.PATTERNS.items():
        assert f'#define TDK_PATTERN_{name} 0x{word:08x}u' in base, name


def test_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    names = ['src', 'dst', 'w', 'h', 'pattern', 'src_dtype', 'dst_dtype', 'flags', 'stream']
    args = [fake, fake + (1 << 24), 640, 480, spec.RGGB, F32, F32, 0, None]

    def fails(needle, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        assert lib.tdk_lmmse(*a) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())
        assert lib.tdk_last_error().startswith(b'tdk_lmmse:')

    for k in ('src', 'dst'):
        fails(b'null pointer (src or dst)', **{k: None})
    for k in ('w', 'h'):
        for v in (1, 0, -2, 65536):
            fails(b'frame size', **{k: v})
    for p in (0, 1, 0x94949495, 0x94941616, 0xFFFFFFFF, 0x55555555):
        fails(b'none of the four Bayer patterns', pattern=p)
    for d in (U8, 3, -1):
        fails(b'unsupported dtype tag', src_dtype=d)
        fails(b'(dst)', dst_dtype=d)
    for f in (2, 3, 4, 256, -1, 1 << 30):
        fails(b'reserved', flags=f)
    plane, frame = 640 * 480 * 4, 640 * 480 * 3 * 4
    for dst in (fake, fake + 64, fake + plane - 4, fake - frame + 4):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + plane // 2 - 2, src_dtype=F16)
    fails(b'src and dst overlap', dst=fake - frame // 2 + 2, dst_dtype=F16)
    # buffers that touch without sharing a byte pass every check -- and would reach the launch: not made here


def test_lds_query(td):
    from torch_darktable._native import lib

    want = 4 * (54 * 54 + 2 * 34 * 50 + 2 * 34 * 42 + 34 * 17)
    for s in (F32, F16):
        for d in (F32, F16):
            for f in (0, LINEAR):
                assert lib.tdk_lmmse_lds_bytes(s, d, f) == want <= 40 * 1024
    for bad in ((U8, F32, 0), (F32, U8, 0), (-1, F32, 0), (F32, F32, 2), (F32, F32, -1)):
        assert lib.tdk_lmmse_lds_bytes(*bad) == 0, bad


def test_package_exports_the_demosaic(td):
    import torch_darktable

    assert torch_darktable.LMMSE is torch_darktable.lmmse.LMMSE
    assert 'LMMSE' in torch_darktable.__all__ and 'lmmse' in torch_darktable.__all__
    assert torch_darktable.lmmse.__all__ == ['LMMSE']
    assert 'LMMSE' not in torch_darktable.debayer.__dict__   # debayer.py stays the reference's surface
    L = torch_darktable.LMMSE
    for name in ('process', 'lds_bytes'):
        assert callable(getattr(L, name)), name
    for name in ('image_size', 'domain', 'bayer_pattern'):
        assert isinstance(getattr(L, name), property), name
    params = inspect.signature(L.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bayer_pattern', 'domain']
    assert params['domain'].kind is inspect.Parameter.KEYWORD_ONLY and params['domain'].default == 'sqrt'
    params = inspect.signature(L.process).parameters
    assert list(params) == ['self', 'mosaic', 'out_dtype'] and params['out_dtype'].default is None
    assert L.TILE == (32, 32)


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    L, P = td.LMMSE, td.BayerPattern
    with pytest.raises(ValueError, match='CUDA'):
        L(torch.device('cpu'), (64, 48), P.RGGB)
    for size in ((1, 48), (64, 0), (65536, 48), (64, 1), (64.5, 48)):
        with pytest.raises(ValueError, match='dimensions must be integers in 2..65535'):
            L(cuda, size, P.RGGB)
    for pattern in (0, 'RGGB', None, spec.RGGB):
        with pytest.raises(TypeError, match='bayer_pattern must be a BayerPattern'):
            L(cuda, (64, 48), pattern)
    for domain in ('log', '', None, 0):
        with pytest.raises(ValueError, match="domain must be 'sqrt' or 'linear'"):
            L(cuda, (64, 48), P.RGGB, domain=domain)
    with pytest.raises(TypeError):
        L(cuda, (64, 48), P.RGGB, 'linear')   # keyword only

    d = L(cuda, (64, 48), P.GBRG)
    assert (d.width, d.height, d.image_size, d.domain, d.bayer_pattern) == (64, 48, (64, 48), 'sqrt', P.GBRG)
    assert repr(d) == "LMMSE(64x48, GBRG, domain='sqrt')"
    lin = L(cuda, (2, 2), P.BGGR, domain='linear')
    assert lin.domain == 'linear' and lin.image_size == (2, 2)
    assert 0 < d.lds_bytes() <= 65536 and d.lds_bytes(torch.float16, torch.float32) == d.lds_bytes() == lin.lds_bytes(torch.float16)
    assert d.lds_bytes(torch.uint8) == 0 and d.lds_bytes(torch.float32, torch.uint8) == 0

    with pytest.raises(TypeError, match='must be a tensor'):
        d.process([[0.0]])
    for shape in ((48,), (48, 64, 3), (48, 64, 1, 1), (48, 64, 2)):
        with pytest.raises(RuntimeError, match=r'must be \(H, W\) or \(H, W, 1\)'):
            d.process(torch.zeros(shape))
    for shape in ((48, 32), (64, 48), (48, 32, 1), (50, 64, 1)):
        with pytest.raises(RuntimeError, match='expected'):
            d.process(torch.zeros(shape))
    for dtype in (torch.float64, torch.uint8, torch.bfloat16, torch.int32):
        with pytest.raises(RuntimeError, match='float32 or float16'):
            d.process(torch.zeros(48, 64, dtype=dtype))
    for dtype in (torch.float64, torch.uint8, torch.bfloat16):
        with pytest.raises(ValueError, match='out_dtype must be float32 or float16'):
            d.process(torch.zeros(48, 64), out_dtype=dtype)
    with pytest.raises(RuntimeError, match='CUDA'):
        d.process(torch.zeros(48, 64))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        d.process(torch.zeros(48, 64, 1, dtype=torch.float16), out_dtype=torch.float32)


def test_pipeline_takes_the_demosaic_as_a_property_only(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.camera_settings import CameraSettings
    from torch_darktable.pipeline.config import Debayer

    assert not any('demosaic' in name or 'lmmse' in name for name in inspect.signature(ImageProcessor.__init__).parameters)
    assert not any('demosaic' in name or 'lmmse' in name for name in inspect.signature(ImageProcessor.from_camera_settings).parameters)
    assert list(inspect.signature(ImageProcessor.__init__).parameters)[-1] == 'raw_correction'
    for model in (ImageProcessingSettings, CameraSettings):
        assert not any('demosaic' in name or 'lmmse' in name for name in model.model_fields), model
    assert sorted(m.name for m in Debayer) == ['bilinear', 'ppg', 'rcd']   # the enum stays the reference's
    assert isinstance(ImageProcessor.demosaic, property) and ImageProcessor.demosaic.fset is not None
    assert ImageProcessor._lmmse is None   # the class-level default
    cuda = torch.device('cuda', 0)
    P = td.BayerPattern
    # an object made without the constructor has the slot through the class: the property needs the size and the pattern only
    p = ImageProcessor.__new__(ImageProcessor)
    p.image_size, p.bayer_pattern = (64, 48), P.GRBG
    assert '_lmmse' not in vars(p) and p.demosaic is None
    for bad in (object(), 3, 'lmmse', td.Sharpen(cuda), td.RCD, td.Deconvolve(cuda, (64, 48))):
        with pytest.raises(TypeError, match='demosaic must be an LMMSE or None'):
            p.demosaic = bad
    for size in ((32, 48), (64, 50), (48, 64)):
        with pytest.raises(ValueError, match=rf'demosaic is for {size[0]}x{size[1]}, the processor for 64x48'):
            p.demosaic = td.LMMSE(cuda, size, P.GRBG)
    for pattern in (P.RGGB, P.BGGR, P.GBRG):
        with pytest.raises(ValueError, match=rf'demosaic is for {pattern.name}, the processor for GRBG'):
            p.demosaic = td.LMMSE(cuda, (64, 48), pattern)
    assert p.demosaic is None
    stage = td.LMMSE(cuda, (64, 48), P.GRBG, domain='linear')
    p.demosaic = stage
    assert p.demosaic is stage and ImageProcessor._lmmse is None
    p.demosaic = None
    assert p.demosaic is None
    # _demosaic asks the stage first and hands it the storage type; load_image leaves the fused RCD path to the reference's methods
    source = inspect.getsource(ImageProcessor._demosaic)
    assert source.index('self._lmmse.process(mosaic, out_dtype=self.storage_dtype)') < source.index('bilinear5x5_demosaic')
    assert source.index('self._lmmse.process') < source.index('self.postprocess_workspace.process(rgb) if self.settings.postprocess else rgb')
    assert 'self.settings.debayer == Debayer.rcd and self._lmmse is None' in inspect.getsource(ImageProcessor.load_image)
