"""CPU-only: the header include/tdk_hip_defringe.h (purple-fringe removal) -- it parses to exactly its five declarations (exports and
the ctypes table: tests/test_header_abi.py), its constants and formulas are the ones the restatement uses, its source is part of the
build's source hash, every argument error of tdk_defringe is reported on the host before any HIP call (the status is the one of an
invalid argument, not of a failed launch, on a machine without a device too), the host queries answer what the documents say, and
the Python front-end torch_darktable.Defringe and the pipeline property raise the error types of the other operators.  The
stand-alone program tests/hip_unit/defringe_arguments_main.cpp makes the same calls for a run under a host sanitizer."""

import ctypes
import inspect
import math
import re
from pathlib import Path

import pytest

import defringe_spec as spec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_defringe.h'
EXPECTED = ['tdk_defringe', 'tdk_defringe_abi_version', 'tdk_defringe_lds_bytes', 'tdk_defringe_weights', 'tdk_defringe_workspace_bytes']
F32, F16, U8 = 0, 1, 2
INVALID_ARGUMENT = 1


def cap(groups):
    return groups << 8


def test_header_declares_the_defringe_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for name, value in (('ABI_VERSION', 1), ('GLOBAL', 0), ('LINEAR', 1), ('STATIC', 2), ('GROUPS_SHIFT', 8), ('GROUPS_MASK', 524032), ('MAX_RADIUS', 12),
                        ('MAX_SAMPLE_RADIUS', 8), ('MAX_GROUPS', 1024), ('TILE', 32), ('STAT_SCALE', 1048576), ('STAT_CAP', 1024)):
        assert re.search(rf'#define TDK_DEFRINGE_{name} {value}\b', text), name
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_defringe'] == ('int', ['const void* src', 'void* dst', 'unsigned char* mask_out', 'float* edge_out', 'tdk_defringe_stats* stats_out',
                                             'void* workspace', 'int width', 'int height', 'int dtype', 'const float* weights', 'int radius', 'int sample_radius',
                                             'float strength', 'float floor', 'int flags', 'tdk_stream_t stream'])
    assert decls['tdk_defringe_weights'] == ('int', ['float sigma', 'float* weights', 'int* radius'])
    assert decls['tdk_defringe_workspace_bytes'] == ('size_t', ['int width', 'int height'])
    assert decls['tdk_defringe_lds_bytes'] == ('size_t', ['int dtype', 'int radius', 'int sample_radius', 'int flags'])
    assert decls['tdk_defringe_abi_version'] == ('int', [])
    assert re.search(r'typedef struct tdk_defringe_stats \{\s*uint64_t sum;.*?float threshold;.*?uint32_t reserved;.*?\} tdk_defringe_stats;', text, flags=re.S)
    for formula in ('p(v) = v > 0 ? v : +0', 't_c = sqrtf(p(x_c))', 't_c = p(x_c)', 'Y  = (0.25f*t_r + 0.5f*t_g) + 0.25f*t_b', 'Cb = t_b - t_g', 'Cr = t_r - t_g',
                    'h = w[0]*s[0]', 'h = h + w[k]*(s[-k] + s[+k])', 'db = Cb - G(Cb)', 'dr = Cr - G(Cr)', 'E  = db*db + dr*dr',
                    'q = (unsigned long long)floorf(fminf(E, 1024.0f) * 1048576.0f)', 'avg = (float)((double)S / ((double)N * 1048576.0))',
                    'th = fmaxf(floor, strength * avg)', 'th = fmaxf(floor, strength)', 'dx*dx + dy*dy <= S_r*S_r', 'dy ascending, then dx ascending',
                    'wt_s = 1.0f / (E_s + th)', 'a = a + wt_s*Cb_s', 'b = b + wt_s*Cr_s', 'n = n + wt_s', "Cb' = a / n", "Cr' = b / n",
                    "g'  = Y - 0.25f*(Cb' + Cr')", "r'  = g' + Cr'", "b'  = g' + Cb'", "v_c = fmaxf(c', 0)", 'out_c = v_c*v_c', 'out_c = v_c ',
                    'stores x_c itself', 'No mirror identity is claimed'):
        assert formula in text, formula
    assert (_native.TDK_DEFRINGE_GLOBAL, _native.TDK_DEFRINGE_LINEAR, _native.TDK_DEFRINGE_STATIC) == (0, 1, 2) == (spec.GLOBAL, spec.LINEAR, spec.STATIC)
    assert (_native.TDK_DEFRINGE_GROUPS_SHIFT, _native.TDK_DEFRINGE_GROUPS_MASK) == (8, 524032) == (spec.GROUPS_SHIFT, spec.GROUPS_MASK)
    assert _native.TDK_DEFRINGE_GROUPS_MASK == (2 * _native.TDK_DEFRINGE_MAX_GROUPS - 1) << 8
    assert (_native.TDK_DEFRINGE_MAX_RADIUS, _native.TDK_DEFRINGE_MAX_SAMPLE_RADIUS, _native.TDK_DEFRINGE_MAX_GROUPS, _native.TDK_DEFRINGE_TILE) == (12, 8, 1024, 32)
    assert (spec.MAX_RADIUS, spec.MAX_SAMPLE_RADIUS, spec.MAX_GROUPS, spec.TILE) == (12, 8, 1024, 32)
    assert (_native.TDK_DEFRINGE_STAT_SCALE, _native.TDK_DEFRINGE_STAT_CAP) == (1048576, 1024) == (int(spec.STAT_SCALE), int(spec.STAT_CAP))
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_defringe.h']
    assert rows == [('tdk_hip_defringe.h', _native.DEFRINGE_SIGNATURES, 'tdk_defringe_abi_version', 1, 'defringe ABI')]
    assert _native.ABI_VERSIONS['tdk_defringe_abi_version'] == (1, 'defringe ABI')
    assert sorted(_native.DEFRINGE_SIGNATURES) == EXPECTED and _native.lib.tdk_defringe_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'defringe.hip') in build._inputs()
    assert [h.name for h in build.HEADERS] == [row[0] for row in _native.HEADERS]


def test_weights_are_the_restatements_and_a_float64_recomputation(td):
    from torch_darktable._native import lib

    buf, radius = (ctypes.c_float * 13)(), ctypes.c_int(-1)
    for sigma in (0.5, 0.7, 1.0, 1.5, 2.0, 2.5, 3.3, 4.0):
        buf[:] = [9.0] * 13
        assert lib.tdk_defringe_weights(sigma, buf, ctypes.byref(radius)) == 0
        taps = spec.gaussian_taps(sigma)
        assert radius.value == len(taps) - 1 and tuple(buf[: len(taps)]) == tuple(float(t) for t in taps) and all(v == 0.0 for v in buf[len(taps):])
        s = ctypes.c_float(sigma).value   # float64 again, written out
        r = math.ceil(3.0 * s)
        raw = [math.exp(-(k * k) / (2.0 * s * s)) for k in range(r + 1)]
        tail = 0.0
        for v in raw[1:]:
            tail += v
        assert radius.value == r and [buf[k] for k in range(r + 1)] == [ctypes.c_float(v / (raw[0] + 2.0 * tail)).value for v in raw]
    for sigma in (0.49, 4.01, 0.0, -1.0, float('nan'), float('inf')):
        assert lib.tdk_defringe_weights(sigma, buf, ctypes.byref(radius)) == 1 and b'tdk_defringe_weights: sigma must lie in [0.5, 4]' in lib.tdk_last_error()
    assert lib.tdk_defringe_weights(2.0, None, ctypes.byref(radius)) == 1 and b'null pointer' in lib.tdk_last_error()
    assert lib.tdk_defringe_weights(2.0, buf, None) == 1 and b'null pointer' in lib.tdk_last_error()


def test_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake, gap = 1 << 30, 1 << 24   # never dereferenced: every check below happens before anything touches device memory or a device
    taps = (ctypes.c_float * 7)(*spec.gaussian_taps(2.0))
    names = ['src', 'dst', 'mask', 'edge', 'stats', 'ws', 'w', 'h', 'dtype', 'weights', 'radius', 'sample_radius', 'strength', 'floor', 'flags', 'stream']
    args = [fake, fake + gap, fake + 2 * gap, fake + 3 * gap, fake + 4 * gap, fake + 5 * gap, 640, 480, F32, taps, 6, 6, 2.5, 1e-4, 0, None]

    def fails(needle, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        assert lib.tdk_defringe(*a) == INVALID_ARGUMENT and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())
        assert lib.tdk_last_error().startswith(b'tdk_defringe:')

    for k in ('src', 'dst'):
        fails(b'null pointer (src or dst)', **{k: None})
    fails(b'null pointer (weights)', weights=None)
    fails(b'null pointer (workspace)', ws=None)
    for k in ('w', 'h'):
        for v in (0, -2, 65536):
            fails(b'frame size', **{k: v})
    for d in (U8, 3, -1):
        fails(b'unsupported dtype', dtype=d)
    for r in (0, -1, 13, 64):
        fails(b'radius must be 1..12', radius=r, weights=(ctypes.c_float * 65)(*([0.01] * 65)))
    for k, bad in enumerate((float('nan'), float('inf'), -0.5, -1e-9)):
        w = [float(t) for t in spec.gaussian_taps(2.0)]
        w[k] = bad
        fails(f'weights[{k}]'.encode(), weights=(ctypes.c_float * 7)(*w))
    for s in (0, -1, 9, 64):
        fails(b'sample_radius must be 1..8', sample_radius=s)
    for s in (-1.0, -1e-9, float('nan'), float('inf')):
        fails(b'strength must be finite and >= 0', strength=s)
    for f in (0.0, -1e-4, float('nan'), float('inf'), 1e-50):   # (1e-50 is 0 as a float32)
        fails(b'floor must be finite and > 0', floor=f)
    for f in (4, 8, 128, 1 << 19, -1, 1 << 30, cap(1025), cap(2047), 3 | 64):
        fails(b'reserved', flags=f)
    fails(b'edge_out must be aligned to 4 bytes', edge=fake + 3 * gap + 2)
    for off in (1, 4, 6):
        fails(b'stats_out must be aligned to 8 bytes', stats=fake + 4 * gap + off)
    # overlap, in bytes of the dtype
    plane = 640 * 480 * 4
    frame = 3 * plane
    need = int(lib.tdk_defringe_workspace_bytes(640, 480))
    for dst in (fake, fake + 64, fake - frame + 4, fake + frame - 4):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + frame // 2 - 2, dtype=F16)
    fails(b'mask_out overlaps src', mask=fake + frame - 1)
    fails(b'mask_out overlaps dst', mask=fake + gap - plane // 4 + 1)
    fails(b'edge_out overlaps src', edge=fake + frame - 4)
    fails(b'edge_out overlaps dst', edge=fake + gap - plane + 4)
    fails(b'edge_out overlaps mask_out', edge=fake + 2 * gap + plane // 4 - 4)
    fails(b'stats_out overlaps src', stats=fake)
    fails(b'stats_out overlaps dst', stats=fake + gap + frame - 8)
    fails(b'stats_out overlaps mask_out', stats=fake + 2 * gap + 8)
    fails(b'stats_out overlaps edge_out', stats=fake + 3 * gap + plane - 8)
    fails(b'the workspace overlaps src', ws=fake + frame - 1)
    fails(b'the workspace overlaps dst', ws=fake + gap - need + 1)
    fails(b'the workspace overlaps mask_out', ws=fake + 2 * gap + 5)
    fails(b'the workspace overlaps edge_out', ws=fake + 3 * gap - 16)
    fails(b'the workspace overlaps stats_out', ws=fake + 4 * gap - need + 8)
    # null optional outputs are not looked at: the same bad argument is reported with and without them
    fails(b'sample_radius must be 1..8', sample_radius=9, mask=None, edge=None, stats=None)
    # every legal flag word, the ends of every range and null optional outputs pass every check -- and would reach the launch: not made here


def test_workspace_and_lds_queries(td):
    from torch_darktable._native import lib

    for w, h in ((640, 480), (641, 481), (1, 1), (3, 3), (65535, 65535)):
        assert lib.tdk_defringe_workspace_bytes(w, h) == spec.workspace_bytes(w, h), (w, h)
    assert lib.tdk_defringe_workspace_bytes(640, 480) == 640 * 480 * 4 + 1024 * 8 + 16
    assert lib.tdk_defringe_workspace_bytes(3, 3) == 48 + 8192 + 16   # the records start on 16 bytes
    for bad in ((0, 480), (640, 65536), (-1, 5), (5, 0)):
        assert lib.tdk_defringe_workspace_bytes(*bad) == 0, bad
    assert spec.lds_bytes() == 39456 <= 40 * 1024 and spec.lds_bytes_correct() == 36912 < spec.lds_bytes()
    for tag in (F32, F16):
        for radius in (1, 6, 12):
            for sample_radius in (1, 6, 8):
                for flags in (0, spec.LINEAR, spec.STATIC, spec.LINEAR | spec.STATIC, cap(1), cap(1024) | spec.STATIC):
                    assert lib.tdk_defringe_lds_bytes(tag, radius, sample_radius, flags) == spec.lds_bytes(), (tag, radius, sample_radius, flags)
    for bad in ((U8, 6, 6, 0), (-1, 6, 6, 0), (F32, 0, 6, 0), (F32, 13, 6, 0), (F32, 6, 0, 0), (F32, 6, 9, 0), (F32, 6, 6, 4), (F32, 6, 6, cap(1025)), (F32, 6, 6, -1)):
        assert lib.tdk_defringe_lds_bytes(*bad) == 0, bad


def test_package_exports_the_stage(td):
    import torch_darktable

    assert torch_darktable.Defringe is torch_darktable.defringe.Defringe
    assert 'Defringe' in torch_darktable.__all__ and 'defringe' in torch_darktable.__all__
    assert torch_darktable.defringe.__all__ == ['Defringe']
    D = torch_darktable.Defringe
    for name in ('process', 'edge', 'threshold', 'workspace_bytes', 'lds_bytes', 'from_weights'):
        assert callable(getattr(D, name)), name
    for name in ('taps', 'blur_radius', 'launches', 'image_size', 'max_groups'):
        assert isinstance(getattr(D, name), property), name
    params = inspect.signature(D.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'sigma', 'radius', 'strength', 'floor', 'mode', 'domain']
    assert [params[k].default for k in list(params)[3:]] == [2.0, 6, 2.5, 1e-4, 'global', 'sqrt']
    params = inspect.signature(D.from_weights).parameters
    assert list(params) == ['device', 'image_size', 'taps', 'radius', 'strength', 'floor', 'mode', 'domain']
    assert [params[k].default for k in list(params)[3:]] == [6, 2.5, 1e-4, 'global', 'sqrt']
    params = inspect.signature(D.process).parameters
    assert list(params) == ['self', 'image', 'return_mask'] and params['return_mask'].default is False
    assert list(inspect.signature(D.edge).parameters) == ['self', 'image'] and list(inspect.signature(D.threshold).parameters) == ['self']
    assert D.TILE == (32, 32)


def test_pipeline_takes_the_stage_as_a_property_only(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.camera_settings import CameraSettings

    assert not any('fring' in name for name in inspect.signature(ImageProcessor.__init__).parameters)
    assert not any('fring' in name for name in inspect.signature(ImageProcessor.from_camera_settings).parameters)
    assert list(inspect.signature(ImageProcessor.__init__).parameters)[-1] == 'raw_correction'
    for model in (ImageProcessingSettings, CameraSettings):
        assert not any('fring' in name for name in model.model_fields), model
    assert isinstance(ImageProcessor.defringe, property) and ImageProcessor.defringe.fset is not None
    assert ImageProcessor._defringe is None   # the class-level default
    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    p = ImageProcessor.__new__(ImageProcessor)
    p.image_size = (64, 48)
    assert '_defringe' not in vars(p) and p.defringe is None
    for bad in (object(), 3, 'defringe', td.Sharpen(cuda), td.Deconvolve(cuda, (64, 48))):
        with pytest.raises(TypeError, match='defringe must be a Defringe or None'):
            p.defringe = bad
    for size in ((32, 48), (64, 50), (48, 64)):
        with pytest.raises(ValueError, match=rf'defringe is for {size[0]}x{size[1]}, the processor for 64x48'):
            p.defringe = td.Defringe(cuda, size)
    assert p.defringe is None
    d = td.Defringe(cuda, (64, 48))
    p.defringe = d
    assert p.defringe is d and ImageProcessor._defringe is None
    p.defringe = None
    assert p.defringe is None
    source = inspect.getsource(ImageProcessor._process_frames)
    assert source.index('self.chroma_denoise.process(img)') < source.index('self._defringe.process') < source.index('self._capture_sharpen.process') < source.index('self.color.process')


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)
    D = td.Defringe
    with pytest.raises(ValueError, match='CUDA'):
        D(torch.device('cpu'), (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions must be 1'):
            D(cuda, size)
    for sigma in (0.49, 4.5, 0.0, float('nan')):
        with pytest.raises(ValueError, match='sigma must lie in'):
            D(cuda, (64, 48), sigma=sigma)
    for radius in (0, 9, 2.5, -1):
        with pytest.raises(ValueError, match='radius must be an integer in 1..8'):
            D(cuda, (64, 48), radius=radius)
    for strength in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='strength must be'):
            D(cuda, (64, 48), strength=strength)
    for floor in (0.0, -0.1, float('nan'), float('inf'), 1e-50):
        with pytest.raises(ValueError, match='floor must be'):
            D(cuda, (64, 48), floor=floor)
    for mode in ('local', 'GLOBAL', None, 0):
        with pytest.raises(ValueError, match='mode must be one of'):
            D(cuda, (64, 48), mode=mode)
    for domain in ('log', 'SQRT', None, 1):
        with pytest.raises(ValueError, match='domain must be one of'):
            D(cuda, (64, 48), domain=domain)
    for taps in ((1.0,), (0.05,) * 14, (0.5, -0.25), (0.5, float('nan'))):
        with pytest.raises(ValueError, match='taps must'):
            D.from_weights(cuda, (64, 48), taps)

    d = D(cuda, (64, 48), sigma=1.5, radius=4, strength=3.0, floor=2e-4, mode='static', domain='linear')
    assert (d.width, d.height, d.image_size, d.blur_radius, d.radius, d.strength, d.mode, d.domain, d.launches) == (64, 48, (64, 48), 5, 4, 3.0, 'static', 'linear', 2)
    assert d.sigma == 1.5 and d.floor == ctypes.c_float(2e-4).value
    assert d.taps == tuple(float(t) for t in spec.gaussian_taps(1.5))
    assert d.workspace_bytes() == 64 * 48 * 4 + 8192 + 16 == spec.workspace_bytes(64, 48)
    assert d._flags() == spec.LINEAR | spec.STATIC and d.max_groups == 1024
    assert repr(d) == "Defringe(64x48, sigma=1.5, blur_radius=5, radius=4, strength=3, floor=0.0002, mode='static', domain='linear')"
    assert d.lds_bytes(torch.float16) == d.lds_bytes() == spec.lds_bytes() and d.lds_bytes(torch.uint8) == 0
    d.max_groups = 2
    assert d.max_groups == 2 and d._flags() == spec.LINEAR | spec.STATIC | cap(2) and d.lds_bytes() == spec.lds_bytes()
    for bad in (-1, 1025):
        with pytest.raises(ValueError, match='max_groups must be'):
            d.max_groups = bad
    d.max_groups = None
    assert d.max_groups == 1024 and d._flags() == 3
    default = D(cuda, (64, 48))
    assert (default.sigma, default.blur_radius, default.radius, default.strength, default.mode, default.domain, default._flags()) == (2.0, 6, 6, 2.5, 'global', 'sqrt', 0)
    own = D.from_weights(cuda, (64, 48), (0.5, 0.25))
    assert own.sigma is None and own.blur_radius == 1 and own.taps == (0.5, 0.25) and 'taps=(0.5, 0.25)' in repr(own)

    with pytest.raises(AssertionError, match='3 dimensions'):
        default.process(torch.zeros(48, 64))
    with pytest.raises(RuntimeError, match='expected'):
        default.process(torch.zeros(48, 32, 3))
    with pytest.raises(ValueError, match='channels must be 1 or 3'):
        default.process(torch.zeros(48, 64, 2))   # (one channel is refused behind the device check: tests/test_gpu_defringe.py)
    with pytest.raises(RuntimeError, match='CUDA'):
        default.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        default.edge(torch.zeros(48, 64, 3))
