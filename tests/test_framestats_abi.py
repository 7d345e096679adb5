"""CPU-only: the header include/tdk_hip_stats.h (frame statistics) -- it parses to exactly its four declarations (exports and the
ctypes table: tests/test_header_abi.py), every argument error of tdk_framestats is reported on the host before any HIP call, the
workspace and LDS queries give the documented sizes, and the Python front-end torch_darktable.FrameStats and the pipeline hook
exist and validate their arguments without a device."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_stats.h'
EXPECTED = ['tdk_framestats', 'tdk_framestats_abi_version', 'tdk_framestats_lds_bytes', 'tdk_framestats_workspace_bytes']
F32, F16, U8, U16 = 0, 1, 2, 3
RGGB = 0x94949494
GRID, CHUNK = 512, 8192


def test_header_declares_the_stats_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_STATS_ABI_VERSION 1', 'TDK_U16 3', 'TDK_STATS_MAX_BINS 1024', 'TDK_STATS_MAX_FRAMES 16', 'TDK_STATS_MAX_QUANTILES 8',
                   f'TDK_STATS_GRID {GRID}', f'TDK_STATS_CHUNK {CHUNK}'):
        assert re.search(rf'#define {define}\b', text), define
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_framestats'] == ('int', ['const void* const* frames', 'int num_frames', 'int dtype', 'void* workspace', 'int width', 'int height',
                                               'int channels', 'uint32_t pattern', 'int stride', 'int bins', 'float lo', 'float hi', 'int min_count',
                                               'const float* quantiles', 'int num_quantiles', 'long long* counts', 'float* values', 'tdk_stream_t stream'])
    assert decls['tdk_framestats_workspace_bytes'] == ('size_t', ['int bins', 'int channels', 'int max_frames'])
    assert decls['tdk_framestats_lds_bytes'] == ('size_t', ['int bins', 'int channels'])
    assert decls['tdk_framestats_abi_version'] == ('int', [])
    for formula in ('t = (x - lo) * scale', 'b = (int) fminf(fmaxf(floorf(t), 0.0f), (float)(B - 1))', 'below[k] += (x < lo);   above[k] += (x >= hi)',
                    'sum[k]   += (long long) rintf(fminf(fmaxf(t, 0.0f), (float)B) * 1048576.0f)', 'scale = fl32(fl32(B) / range)',
                    'mean[k] = valid[k] >= min_count ? (float)((double)lo + ((double)sum[k] / ((double)valid[k] * 1048576.0)) * w) : 0.0f',
                    'r = ceil((double)q * (double)N) clamped to [1, N]', 'frac = (double)(r - cum(b* - 1)) / (double)H[b*]',
                    'value = (float)((double)lo + ((double)b* + frac) * w)', 'gain[k] = fminf(fmaxf(mean[1] / mean[k], 1.0f/64.0f), 64.0f)',
                    'a NaN never reaches the index conversion'):
        assert formula in text, formula
    assert _native.TDK_U16 == U16 and (_native.TDK_F32, _native.TDK_F16, _native.TDK_U8) == (F32, F16, U8)
    assert (_native.TDK_STATS_MAX_BINS, _native.TDK_STATS_MAX_FRAMES, _native.TDK_STATS_MAX_QUANTILES) == (1024, 16, 8)
    assert (_native.TDK_STATS_GRID, _native.TDK_STATS_CHUNK) == (GRID, CHUNK)
    assert _native.ABI_VERSIONS['tdk_framestats_abi_version'] == (1, 'stats ABI')
    assert _native.lib.tdk_framestats_abi_version() == 1
    assert 'tdk_hip_stats.h' in [row[0] for row in _native.HEADERS]


def test_framestats_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    frames = (ctypes.c_void_p * 2)(fake, fake + (1 << 24))
    q = (ctypes.c_float * 3)(0.001, 0.5, 0.999)
    workspace, counts, values = fake + (1 << 26), fake + (2 << 26) + (1 << 25), fake + (3 << 26)
    names = ['frames', 'num_frames', 'dtype', 'workspace', 'width', 'height', 'channels', 'pattern', 'stride', 'bins', 'lo', 'hi', 'min_count', 'quantiles',
             'num_quantiles', 'counts', 'values', 'stream']
    args = [frames, 2, F32, workspace, 640, 480, 3, 0, 1, 256, 0.0, 1.0, 64, q, 3, counts, values, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_framestats(*a)

    def rejected(word, **change):
        return call(**change) == 1 and word in lib.tdk_last_error()

    for k in ('frames', 'workspace', 'counts', 'values'):
        assert rejected(b'null pointer', **{k: None}), k
    assert rejected(b'frames[1]', frames=(ctypes.c_void_p * 2)(fake, None))
    assert rejected(b'null pointer (quantiles)', quantiles=None)
    for v in (0, -1, 17):
        assert rejected(b'num_frames', num_frames=v), v
    for v in (4, -1, 9):
        assert rejected(b'dtype', dtype=v), v
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
    for v in (0, 2, 4, -1):
        assert rejected(b'channels', channels=v), v
    assert rejected(b'Bayer pattern', pattern=0x12345678) and rejected(b'Bayer pattern', pattern=1)
    assert rejected(b'channels = 3', pattern=RGGB, channels=1)
    assert rejected(b'even', pattern=RGGB, width=641) and rejected(b'even', pattern=RGGB, height=479)
    for v in (0, -1, 65536):
        assert rejected(b'stride', stride=v), v
    for v in (1, 0, -5, 1025):
        assert rejected(b'bins', bins=v), v
    for lo, hi in ((1.0, 1.0), (1.0, 0.0), (float('nan'), 1.0), (0.0, float('nan')), (0.0, float('inf')), (-float('inf'), 0.0), (-3e38, 3e38), (0.0, 1e-44)):
        assert rejected(b'range', lo=lo, hi=hi), (lo, hi)
    for v in (0, -1):
        assert rejected(b'min_count', min_count=v), v
    for v in (-1, 9):
        assert rejected(b'num_quantiles', num_quantiles=v), v
    for bad in (-0.001, 1.001, float('nan'), float('inf')):
        assert rejected(b'quantiles[1]', quantiles=(ctypes.c_float * 3)(0.0, bad, 1.0)), bad
    assert rejected(b'aligned to 8', counts=counts + 4)
    frame_bytes = 640 * 480 * 3 * 4
    for k in ('workspace', 'counts', 'values'):
        assert rejected(b'frames[0] overlaps', **{k: fake + 64}), k
        assert rejected(b'frames[1] overlaps', **{k: fake + (1 << 24) + frame_bytes - 8}), k
    ws_bytes = lib.tdk_framestats_workspace_bytes(256, 3, 2)
    assert rejected(b'overlap', counts=workspace + ws_bytes - 8) and rejected(b'overlap', values=counts + 8)
    # a mosaic frame is width * height elements: what lies behind them may be anything
    assert rejected(b'frames[0] overlaps', pattern=RGGB, dtype=U8, counts=fake + 640 * 480 - 8)


def test_workspace_and_lds_queries(td):
    from torch_darktable._native import lib

    ws, lds = lib.tdk_framestats_workspace_bytes, lib.tdk_framestats_lds_bytes
    for bad in ((1, 3, 1), (1025, 3, 1), (256, 2, 1), (256, 0, 1), (256, 3, 0), (256, 3, 17), (-4, 1, 1)):
        assert ws(*bad) == 0, bad
    for bad in ((1, 3), (1025, 1), (256, 2), (256, 4), (0, 0)):
        assert lds(*bad) == 0, bad

    def record(bins, channels):   # uint32 bins padded to an even count, then 5 counters of 8 bytes per channel
        return (channels * bins + 1) // 2 * 2 * 4 + 5 * channels * 8

    for bins in (2, 3, 255, 256, 1000, 1024):
        for channels in (1, 3):
            for frames in (1, 3, 16):
                assert ws(bins, channels, frames) == frames * GRID * record(bins, channels) + 8, (bins, channels, frames)
            assert record(bins, channels) % 8 == 0
    assert ws(256, 3, 1) == GRID * (3072 + 120) + 8 and ws(1024, 3, 16) < 128 << 20
    # the LDS of the gather launch is a constant: sixteen copies of 3 x 256 bins (a multiple of 32 words plus one apart), 16 counters
    sizes = {lds(b, c) for b in (2, 17, 256, 1024) for c in (1, 3)}
    assert sizes == {16 * (3 * 256 + 1) * 4 + 16 * 8} and max(sizes) <= 64 * 1024
    assert 2 * max(sizes) <= 160 * 1024   # two workgroups share a compute unit


def test_package_exports_framestats(td):
    import torch_darktable

    assert torch_darktable.FrameStats is torch_darktable.framestats.FrameStats
    assert torch_darktable.FrameStatistics is torch_darktable.framestats.FrameStatistics
    assert {'FrameStats', 'FrameStatistics', 'framestats'} <= set(torch_darktable.__all__)
    assert torch_darktable.framestats.__all__ == ['FrameStats', 'FrameStatistics']
    assert (torch_darktable.FrameStats.GRID, torch_darktable.FrameStats.CHUNK) == (GRID, CHUNK)
    for name in ('measure', 'bounds', 'white_balance', 'lds_bytes', 'workspace_bytes'):
        assert callable(getattr(torch_darktable.FrameStats, name)), name
    params = inspect.signature(torch_darktable.FrameStats.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'channels', 'bayer_pattern', 'bins', 'value_range', 'stride', 'quantiles', 'max_frames', 'min_count']
    assert [params[k].default for k in ('channels', 'bayer_pattern', 'bins', 'value_range', 'stride', 'quantiles', 'max_frames', 'min_count')] == \
        [3, None, 256, (0.0, 1.0), 1, (0.001, 0.5, 0.999), 1, 64]
    fields = list(torch_darktable.FrameStatistics.__dataclass_fields__)
    assert fields == ['hist', 'below', 'above', 'nan', 'valid', 'sum', 'mean', 'percentiles', 'gains']


def test_pipeline_takes_exposure(td):
    import torch
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor

    params = inspect.signature(ImageProcessor.__init__).parameters
    assert 'exposure' in params and params['exposure'].default is None
    dev = torch.device('cuda', 0)
    build = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None, **kw)
    for wrong in (object(), (0.001, 0.999), 'percentile', td.Sharpen(dev)):
        with pytest.raises(TypeError, match='exposure must be a FrameStats'):
            build(exposure=wrong)
    with pytest.raises(ValueError, match='exposure is for 32x48'):
        build(exposure=td.FrameStats(dev, (32, 48)))
    with pytest.raises(ValueError, match='channels=3'):
        build(exposure=td.FrameStats(dev, (64, 48), channels=1))
    with pytest.raises(ValueError, match='channels=3'):
        build(exposure=td.FrameStats(dev, (64, 48), bayer_pattern=td.BayerPattern.RGGB))
    with pytest.raises(ValueError, match='at least one quantile'):
        build(exposure=td.FrameStats(dev, (64, 48), quantiles=()))
    assert 'exposure' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    for model in (ImageProcessingSettings, CameraSettings):
        assert not {'exposure', 'framestats', 'frame_stats', 'histogram', 'percentile'} & set(model.model_fields), model


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: nothing below needs a GPU
    with pytest.raises(ValueError, match='CUDA'):
        td.FrameStats(torch.device('cpu'), (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            td.FrameStats(cuda, size)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='even'):
            td.FrameStats(cuda, size, bayer_pattern=td.BayerPattern.GRBG)
    with pytest.raises(ValueError, match='bayer pattern'):
        td.FrameStats(cuda, (64, 48), bayer_pattern='RGGB')
    with pytest.raises(ValueError, match='channels = 3'):
        td.FrameStats(cuda, (64, 48), channels=1, bayer_pattern=td.BayerPattern.RGGB)
    for channels in (0, 2, 4):
        with pytest.raises(ValueError, match='channels must be 1 or 3'):
            td.FrameStats(cuda, (64, 48), channels=channels)
    for bins in (1, 1025, 2.5, 0):
        with pytest.raises(ValueError, match='bins'):
            td.FrameStats(cuda, (64, 48), bins=bins)
    for value_range in ((0.0, 0.0), (1.0, 0.0), (0.0, float('inf')), (float('nan'), 1.0), (-3e38, 3e38), (0.0, 1.0, 2.0), (1.0, 1.0 + 1e-12)):
        with pytest.raises(ValueError, match='value_range'):
            td.FrameStats(cuda, (64, 48), value_range=value_range)
    for stride in (0, -1, 1.5, 65536):
        with pytest.raises(ValueError, match='stride'):
            td.FrameStats(cuda, (64, 48), stride=stride)
    for quantiles in ((-0.1,), (1.1,), (float('nan'),), tuple([0.5] * 9)):
        with pytest.raises(ValueError, match='quantiles'):
            td.FrameStats(cuda, (64, 48), quantiles=quantiles)
    for max_frames in (0, 17, 1.5):
        with pytest.raises(ValueError, match='max_frames'):
            td.FrameStats(cuda, (64, 48), max_frames=max_frames)
    for min_count in (0, -3, 2.5):
        with pytest.raises(ValueError, match='min_count'):
            td.FrameStats(cuda, (64, 48), min_count=min_count)

    # what the object tells: the float32 numbers the kernel is given
    fs = td.FrameStats(cuda, (64, 48), value_range=(0.1, 0.9), quantiles=(0.001, 0.999), max_frames=3)
    f = np.float32
    assert fs.image_size == (64, 48) and fs.value_range == (float(f(0.1)), float(f(0.9))) and fs.quantiles == (float(f(0.001)), float(f(0.999)))
    assert (fs.channels, fs.bins, fs.stride, fs.max_frames, fs.min_count, fs.bayer_pattern) == (3, 256, 1, 3, 64, None)
    assert fs.lds_bytes() == 16 * 769 * 4 + 128 and fs.workspace_bytes() == 3 * GRID * 3192 + 8
    assert repr(fs) == 'FrameStats(64x48, 3 channels, bins=256, range=(0.1, 0.9), stride=1, quantiles=(0.001, 0.999), max_frames=3, min_count=64)'
    mosaic = td.FrameStats(cuda, (64, 48), bayer_pattern=td.BayerPattern.BGGR, bins=1024, value_range=(0, 4096), stride=4)
    assert mosaic.channels == 3 and repr(mosaic).startswith('FrameStats(64x48, BGGR, bins=1024, range=(0, 4096), stride=4')

    with pytest.raises(RuntimeError, match='shape'):
        fs.measure(torch.zeros(48, 64))
    with pytest.raises(RuntimeError, match='shape'):
        mosaic.measure(torch.zeros(48, 64, 3))
    with pytest.raises(ValueError, match='max_frames'):
        fs.measure([torch.zeros(48, 64, 3)] * 4)
    with pytest.raises(ValueError, match='max_frames'):
        fs.measure([])
    with pytest.raises(RuntimeError, match='CUDA'):
        fs.measure(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(ValueError, match='three channels'):
        td.FrameStats(cuda, (64, 48), channels=1).white_balance(torch.zeros(48, 64, 1))
    with pytest.raises(ValueError, match='quantile'):
        td.FrameStats(cuda, (64, 48), quantiles=()).bounds(torch.zeros(48, 64, 3))
