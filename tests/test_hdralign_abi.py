"""CPU-only: the header include/tdk_hip_hdralign.h (exposure brackets of a moving rig) -- it parses to exactly its four declarations
(exports and the ctypes table: tests/test_header_abi.py), its row stands directly behind tdk_hip_hdr.h in both registries, every
argument error of tdk_hdralign_pyramid and tdk_hdralign_merge is reported on the host before any HIP call, the LDS query gives the
documented size, and the Python front-end torch_darktable.MotionHdrMerge exists and validates its arguments without a device.  The
stand-alone program tests/hip_unit/hdralign_arguments_main.cpp makes the same calls for a run under a host sanitizer."""

import ctypes
import inspect
import re
from pathlib import Path

import pytest

import hdralign_spec as spec
import hdrmerge_spec as hspec
from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_hdralign.h'
EXPECTED = ['tdk_hdralign_abi_version', 'tdk_hdralign_lds_bytes', 'tdk_hdralign_merge', 'tdk_hdralign_pyramid']
F32, F16, U8, U16 = 0, 1, 2, 3
RGGB = 0x94949494


def test_header_declares_the_hdralign_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_HDRALIGN_ABI_VERSION 1(?!\d)', text)
    for include in ('"tdk_hip.h"', '"tdk_hip_hdr.h"', '"tdk_hip_motion.h"'):
        assert f'#include {include}' in text, include
    assert 'extern "C"' in text
    merge = declarations(ROOT / 'include' / 'tdk_hip_hdr.h')['tdk_hdr_merge']
    assert decls['tdk_hdralign_merge'] == (merge[0], merge[1][:-1] + ['const int16_t* fields', 'tdk_stream_t stream'])   # every argument of tdk_hdr_merge
    assert decls['tdk_hdralign_pyramid'] == ('int', ['const void* src', 'int src_dtype', 'int width', 'int height', 'float scale', 'int levels', 'void* pyramid',
                                                     'int which', 'const float* exposures', 'int num_frames', 'int frame', 'tdk_stream_t stream'])
    assert decls['tdk_hdralign_lds_bytes'] == ('size_t', ['int radius'])
    assert decls['tdk_hdralign_abi_version'] == ('int', [])
    for formula in ('s    = scale * (e_hi / exposures[frame])', 'a later frame replaces an earlier one', 'a NaN ratio gives grey 0',
                    'ref is a frame index, 0..F-1; -1 is refused', 'fields is F x Ty x Tx x 2 int16 on a 4-byte boundary',
                    'D_f = fields[f][i / 32][j / 64] & ~1 for f != ref, and D_ref = 0', 'The row of ref is never read', 'any int16 is memory-safe',
                    "the frame's sample at q + D_f if that lies inside the frame, else NaN", 'takes g = lo when q + D_lo lies inside the frame, else g = ref',
                    'With all-zero fields and ref >= 0 the function is tdk_hdr_merge bit for bit, mask included', 'With finite samples no\n * out is NaN',
                    'lies inside one 64 x 32 motion tile', 'lives in the coordinates of ref', 'tdk_motion_match (tdk_hip_motion.h), unchanged, with index == NULL'):
        assert formula in text, formula
    assert _native.ABI_VERSIONS['tdk_hdralign_abi_version'] == (1, 'hdr alignment ABI')
    assert _native.lib.tdk_hdralign_abi_version() == 1


def test_the_row_stands_directly_behind_the_merge_in_both_registries(td):
    from torch_darktable import _native

    names = [row[0] for row in _native.HEADERS]
    at = names.index('tdk_hip_hdralign.h')
    assert names[at - 1] == 'tdk_hip_hdr.h' and names[-1] == 'tdk_hip_lut.h'
    assert _native.HEADERS[at] == ('tdk_hip_hdralign.h', _native.HDRALIGN_SIGNATURES, 'tdk_hdralign_abi_version', 1, 'hdr alignment ABI')
    assert sorted(_native.HDRALIGN_SIGNATURES) == EXPECTED
    built = [p.name for p in load_build_module().HEADERS]
    assert built == names


def test_merge_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    w, h, nf = 640, 480, 3
    step = 1 << 24   # more than a float32 frame
    out, mask, exposures, model, fields = fake + 8 * step, fake + 9 * step, fake + 10 * step, fake + 10 * step + 64, fake + 11 * step
    frame_at = [fake + f * step for f in range(8)]
    names = ['frames', 'num_frames', 'src_dtype', 'out', 'out_dtype', 'mask', 'width', 'height', 'pattern', 'exposures', 'ref', 'model', 'radius', 'clip', 't_lo',
             't_hi', 'pixel_c2', 'v_min', 'fields', 'stream']

    def call(frames=frame_at, **change):
        args = [(ctypes.c_void_p * len(frames))(*frames) if frames is not None else None, nf, F32, out, F16, mask, w, h, RGGB, exposures, 0, model, 2, 0.95, 1.5, 3.0,
                16.0, 1e-12, fields, None]
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.tdk_hdralign_merge(*args)

    def rejected(word, frames=frame_at, **change):
        return call(frames, **change) == 1 and word in lib.tdk_last_error() and b'tdk_hdralign_merge' in lib.tdk_last_error()

    assert rejected(b'null pointer', frames=None)
    for k in ('out', 'exposures', 'model'):
        assert rejected(b'null pointer', **{k: None}), k
    assert rejected(b'null pointer (fields)', fields=None)
    for f in range(nf):
        assert rejected(b'null pointer (frame', frames=[None if i == f else p for i, p in enumerate(frame_at)]), f
    for v in (1, 0, 9, -1):
        assert rejected(b'num_frames', num_frames=v), v
    for k in ('src_dtype', 'out_dtype'):
        for v in (U8, U16, -1):
            assert rejected(b'dtype', **{k: v}), (k, v)
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        for v in (641, 65535):
            assert rejected(b'even', **{k: v}), (k, v)
    assert rejected(b'Bayer pattern', pattern=0x12345678) and rejected(b'Bayer pattern', pattern=0)
    for v in (1, 0, 4, -2):
        assert rejected(b'radius', radius=v), v
    for v in (-1, -2, 3, 8):   # -1 is refused here: the host says which frame the others follow
        assert rejected(b'ref', ref=v), v
    nan, inf = float('nan'), float('inf')
    for v in (0.0, -1.0, nan, inf):
        assert rejected(b'clip', clip=v), v
    for lo, hi in ((0.0, 3.0), (-1.0, 3.0), (3.0, 3.0), (3.0, 1.5), (nan, 3.0), (1.5, nan), (1.5, inf), (1e-40, 2e-40)):
        assert rejected(b'thresholds', t_lo=lo, t_hi=hi), (lo, hi)
    for v in (0.0, -1.0, nan, -inf):
        assert rejected(b'pixel_c2', pixel_c2=v), v
    for v in (0.0, -1e-12, nan, inf):
        assert rejected(b'v_min', v_min=v), v
    for f in range(nf):
        assert rejected(b'overlaps frame', out=frame_at[f] + 64) and rejected(b'overlaps frame', mask=frame_at[f] + w * h * 4 - 1), f
    assert rejected(b'the exposures or the model overlap', exposures=out + 16) and rejected(b'the exposures or the model overlap', model=mask + w * h - 1)
    assert rejected(b'out and mask overlap', mask=out + w * h * 2 - 1)
    for v in (fields + 1, fields + 2, fields + 3):
        assert rejected(b'fields must be aligned', fields=v), v
    field_bytes = nf * 10 * 15 * 4   # F x Tx x Ty displacements of two int16
    assert rejected(b'the fields overlap', fields=out + 64) and rejected(b'the fields overlap', fields=out - field_bytes + 4)
    assert rejected(b'the fields overlap', fields=mask + w * h - 4) and rejected(b'the fields overlap', fields=mask - field_bytes + 4)
    assert rejected(b'null pointer', out=None, mask=None)   # mask may be NULL, out may not


def test_pyramid_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30
    w, h = 640, 480
    src, pyramid, exposures = fake, fake + (1 << 24), fake + (2 << 24)
    names = ['src', 'src_dtype', 'width', 'height', 'scale', 'levels', 'pyramid', 'which', 'exposures', 'num_frames', 'frame', 'stream']

    def rejected(word, **change):
        args = [src, F32, w, h, 0.25, 3, pyramid, 0, exposures, 3, 1, None]
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.tdk_hdralign_pyramid(*args) == 1 and word in lib.tdk_last_error() and b'tdk_hdralign_pyramid' in lib.tdk_last_error()

    for k in ('src', 'pyramid'):
        assert rejected(b'null pointer', **{k: None}), k
    assert rejected(b'null pointer (exposures)', exposures=None)
    for v in (U8, U16, -1):
        assert rejected(b'dtype', src_dtype=v), v
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        assert rejected(b'even', **{k: 641}), k
    for v in (0.0, -0.25, float('nan'), float('inf')):
        assert rejected(b'scale', scale=v), v
    for v in (0, 5, -1):
        assert rejected(b'levels', levels=v), v
    for v in (2, -1):
        assert rejected(b'which', which=v), v
    assert rejected(b'aligned to 16', pyramid=pyramid + 8)
    for v in (1, 0, 9):
        assert rejected(b'num_frames', num_frames=v), v
    for v in (-1, 3, 8):
        assert rejected(b'frame must be', frame=v), v
    assert rejected(b'exposures must be aligned', exposures=exposures + 2)
    assert rejected(b'src and pyramid overlap', pyramid=src + 1024)
    assert rejected(b'exposures and pyramid overlap', exposures=pyramid + 64)


def test_lds_query(td):
    from torch_darktable._native import lib

    for bad in (0, 1, 4, -2):
        assert lib.tdk_hdralign_lds_bytes(bad) == 0, bad
    for r in (2, 3):
        assert lib.tdk_hdralign_lds_bytes(r) == spec.lds_bytes(r) == lib.tdk_hdr_lds_bytes(r) + 64 == hspec.lds_bytes(r) + 64
    assert lib.tdk_hdralign_lds_bytes(3) <= 64 * 1024


def test_package_exports_the_aligned_merge(td):
    import torch_darktable

    cls = torch_darktable.MotionHdrMerge
    assert cls is torch_darktable.hdralign.MotionHdrMerge and issubclass(cls, torch_darktable.HdrMerge)
    assert {'MotionHdrMerge', 'hdralign'} <= set(torch_darktable.__all__)
    assert torch_darktable.hdralign.__all__ == ['MotionHdrMerge']
    params = inspect.signature(cls.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bayer_pattern', 'noise_model', 'motion', 'kwargs'] and params['motion'].default is None
    params = inspect.signature(cls.process).parameters
    assert list(params) == ['self', 'frames', 'exposures', 'ref', 'out_dtype', 'return_mask', 'fields']
    assert [params[k].default for k in ('ref', 'out_dtype', 'return_mask', 'fields')] == [None, None, False, None]
    assert list(inspect.signature(cls.align).parameters) == ['self', 'frames', 'exposures', 'ref']
    for name in ('fields', 'costs', 'prepare', 'align'):
        assert callable(getattr(cls, name)), name
    assert torch_darktable.hdralign.DEFAULT_ZERO_BIAS == spec.DEFAULT_ZERO_BIAS
    assert 'raw mosaics only' in torch_darktable.hdralign.__doc__


def test_python_front_end_validates_without_a_device(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor

    cuda, cpu = torch.device('cuda', 0), torch.device('cpu')   # a device object only: nothing below needs a GPU
    P = td.BayerPattern.GRBG
    model = td.NoiseModel.from_values((2e-4, 5e-5, 1e-3), 1e-6, cpu)
    with pytest.raises(ValueError, match='CUDA'):
        td.MotionHdrMerge(cpu, (128, 64), P, model)
    with pytest.raises(ValueError, match='even'):
        td.MotionHdrMerge(cuda, (127, 64), P, model)
    with pytest.raises(ValueError, match='radius'):
        td.MotionHdrMerge(cuda, (128, 64), P, model, radius=4)
    for wrong in (object(), 'motion', model):
        with pytest.raises(TypeError, match='motion must be a MotionEstimate'):
            td.MotionHdrMerge(cuda, (128, 64), P, model, motion=wrong)
    with pytest.raises(ValueError, match='motion is for'):
        td.MotionHdrMerge(cuda, (128, 64), P, model, motion=td.MotionEstimate(cuda, (128, 66)))

    t = td.MotionHdrMerge(cuda, (130, 66), P, model, radius=3, clip=0.9)
    assert isinstance(t.motion, td.MotionEstimate) and t.motion.zero_bias == spec.DEFAULT_ZERO_BIAS and t.motion.image_size == (130, 66)
    assert t.radius == 3 and t.lds_bytes() == spec.lds_bytes(3)
    assert repr(t).startswith('MotionHdrMerge(130x66, GRBG, radius=3, clip=0.9') and 'motion=MotionEstimate(130x66' in repr(t)
    own = td.MotionEstimate(cuda, (130, 66), levels=2, search=2, zero_bias=10)
    assert td.MotionHdrMerge(cuda, (130, 66), P, model, motion=own).motion is own
    frame = torch.zeros(66, 130)
    with pytest.raises(ValueError, match='2..8 frames'):
        t.process([frame], (1.0,))
    with pytest.raises(ValueError, match='2..8 frames'):
        t.prepare(1)
    with pytest.raises(RuntimeError, match='shape'):
        t.process([frame, torch.zeros(64, 130)], (1.0, 0.5))
    for ref in (-1, 2, 0.5, True):
        with pytest.raises(ValueError, match='ref'):
            t.process([frame, frame], (1.0, 0.5), ref=ref)
    with pytest.raises(ValueError, match='exposures'):
        t.process([frame, frame], (1.0, 0.0))
    with pytest.raises(ValueError, match='ref=None needs exposures the host holds'):   # the host must know which frame the others follow
        t.process([frame, frame], torch.ones(2), ref=None)
    with pytest.raises(RuntimeError, match='fields must be a contiguous'):
        t.process([frame, frame], (1.0, 0.5), fields=torch.zeros(2, 3, 3, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='fields must be a contiguous'):
        t.process([frame, frame], (1.0, 0.5), fields=torch.zeros(2, 2, 3, 2, dtype=torch.int16))
    with pytest.raises(RuntimeError, match='no bracket has been aligned'):
        t.fields()
    with pytest.raises(RuntimeError, match='CUDA'):
        t.process([frame, frame], (1.0, 0.5))   # no CPU fallback
    assert t._resolve((0.25, 1.0, 1.0, 0.5), None, 4) == 1 and t._resolve((0.25, 1.0), 0, 2) == 0   # the largest exposure, the lowest index

    # the pipeline takes it where it takes an HdrMerge
    proc = ImageProcessor((130, 66), P, td.PackedFormat.Packed12, ImageProcessingSettings(), cuda, None, hdr=t)
    assert proc.hdr is t
