"""Frame statistics (include/tdk_hip_stats.h: tdk_framestats) -- the block of an ISP that measures: per-channel histograms, the
counts below and above the range, percentiles, means and grey-world gains of a frame or of a set of frames, all as device tensors.

    frame     an (H, W, C) image, C = 1 or 3, or an (H, W) mosaic (bayer_pattern given: three channels by colour, the greens pooled)
    storage   float32, float16, uint8 or uint16; integers count at their integer value (a byte histogram: value_range=(0, 256), bins=256)
    stride    every stride-th pixel of every stride-th row (mosaic: CFA cells); rows in between are not read
    a set     up to max_frames frames pool into one result, as compute_image_bounds pools the cameras of an image set

The exact formulas are in the header; a NumPy restatement (tests/framestats_spec.py) predicts every integer and every float bit.
One gather launch per frame and two small finishing launches on PyTorch's current stream; no atomics on global memory, no memset,
no copy, no synchronisation.  The workspace belongs to the object, one per stream, and is never cleared: capturable in a HIP graph
from the first call, and bit-reproducible.

    fs = FrameStats(device, (4096, 3072), channels=3, quantiles=(0.001, 0.5, 0.999), max_frames=6)
    bounds = fs.bounds(rgb_frames)                         # (2,) float32: the percentile bounds normalize_image takes
    wb = FrameStats(device, (4096, 3072), bayer_pattern=BayerPattern.RGGB, stride=4)
    mosaic = apply_white_balance(raw, wb.white_balance(raw), BayerPattern.RGGB)   # the gains never leave the device
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from ._frames import MAX_SIZE
from ._mosaic import MosaicStage, check_pattern
from ._native import (TDK_F16, TDK_F32, TDK_STATS_CHUNK, TDK_STATS_GRID, TDK_STATS_MAX_BINS, TDK_STATS_MAX_FRAMES, TDK_STATS_MAX_QUANTILES, TDK_U8, TDK_U16,
                      check, lib)
from ._stage import as_float32 as _f32
from .bayer import BayerPattern
from .torch_darktable_extension import _pattern, _ptr, _require, _stream

_TAGS = {torch.float32: TDK_F32, torch.float16: TDK_F16, torch.uint8: TDK_U8, torch.uint16: TDK_U16}
_COUNTERS = 5  # below, above, nan, valid, sum


@dataclass
class FrameStatistics:
    """What `FrameStats.measure` returns; every tensor is on the device.  C channels, B bins, Q quantiles."""

    hist: torch.Tensor          # (C, B) int64
    below: torch.Tensor         # (C,) int64: sampled values < lo
    above: torch.Tensor         # (C,) int64: sampled values >= hi
    nan: torch.Tensor           # (C,) int64
    valid: torch.Tensor         # (C,) int64: members of groups with every member inside [lo, hi)
    sum: torch.Tensor           # (C,) int64: their positions in the range in units of bin_width / 2**20
    mean: torch.Tensor          # (C,) float32; 0 below min_count
    percentiles: torch.Tensor   # (C + 1, Q) float32; the last row is the pooled histogram
    gains: torch.Tensor         # (3,) float32 grey-world gains (R, G, B), green = 1


class FrameStats(MosaicStage):
    """Measure frames of one size; image_size is (width, height).  `channels` (1 or 3) is for (H, W, C) images; with `bayer_pattern`
    the frames are (H, W) mosaics, width and height even, and the result has three channels."""

    GRID = TDK_STATS_GRID    # workgroups of the gather launch, whatever the frame size (csrc/framestats.hip: FS_GRID)
    CHUNK = TDK_STATS_CHUNK  # pixels a workgroup takes per step: a frame beyond GRID * CHUNK pixels makes every workgroup loop

    def __init__(self, device: torch.device, image_size: tuple[int, int], channels: int = 3, bayer_pattern: BayerPattern | None = None, bins: int = 256,
                 value_range: tuple[float, float] = (0.0, 1.0), stride: int = 1, quantiles=(0.001, 0.5, 0.999), max_frames: int = 1, min_count: int = 64):
        super().__init__(device, image_size, min_size=1)
        if bayer_pattern is not None:
            check_pattern(bayer_pattern)
            self._check_even()
            if channels != 3:
                raise ValueError(f'a mosaic has channels = 3 (R, G, B), got {channels}')
        if channels not in (1, 3):
            raise ValueError(f'channels must be 1 or 3, got {channels}')
        if int(bins) != bins or not 2 <= int(bins) <= TDK_STATS_MAX_BINS:
            raise ValueError(f'bins must be an integer in 2..{TDK_STATS_MAX_BINS}, got {bins}')
        if len(tuple(value_range)) != 2:
            raise ValueError(f'value_range must be (lo, hi), got {value_range}')
        lo, hi = _f32(value_range[0]), _f32(value_range[1])
        span = _f32(hi - lo) if math.isfinite(lo) and math.isfinite(hi) else math.nan
        if not (lo < hi and math.isfinite(span) and math.isfinite(_f32(float(int(bins)) / span))):
            raise ValueError(f'value_range must be finite with lo < hi, got {tuple(value_range)}')
        if int(stride) != stride or not 1 <= int(stride) <= MAX_SIZE:
            raise ValueError(f'stride must be an integer in 1..{MAX_SIZE}, got {stride}')
        q = tuple(float(v) for v in quantiles)
        if len(q) > TDK_STATS_MAX_QUANTILES or not all(0.0 <= v <= 1.0 for v in q):
            raise ValueError(f'quantiles must be at most {TDK_STATS_MAX_QUANTILES} fractions in [0, 1], got {tuple(quantiles)}')
        if int(max_frames) != max_frames or not 1 <= int(max_frames) <= TDK_STATS_MAX_FRAMES:
            raise ValueError(f'max_frames must be an integer in 1..{TDK_STATS_MAX_FRAMES}, got {max_frames}')
        if int(min_count) != min_count or not 1 <= int(min_count) < 2 ** 31:
            raise ValueError(f'min_count must be an integer >= 1, got {min_count}')
        self.channels, self.bayer_pattern = int(channels), bayer_pattern
        self.bins, self.lo, self.hi, self.stride = int(bins), lo, hi, int(stride)
        self.quantiles = tuple(_f32(v) for v in q)   # the float32 fractions the kernel is given
        self.max_frames, self.min_count = int(max_frames), int(min_count)
        self._c_quantiles = (ctypes.c_float * max(len(q), 1))(*self.quantiles)
        self._keep_workspace()

    @property
    def value_range(self) -> tuple[float, float]:
        return (self.lo, self.hi)

    def __repr__(self):
        kind = self.bayer_pattern.name if self.bayer_pattern is not None else f'{self.channels} channel{"s" if self.channels > 1 else ""}'
        return (f'FrameStats({self.width}x{self.height}, {kind}, bins={self.bins}, range=({self.lo:g}, {self.hi:g}), stride={self.stride}, '
                f'quantiles={tuple(round(v, 6) for v in self.quantiles)}, max_frames={self.max_frames}, min_count={self.min_count})')

    def lds_bytes(self) -> int:
        """LDS of a workgroup of the gather launch: the replicated histograms and the counters."""
        return int(lib.tdk_framestats_lds_bytes(self.bins, self.channels))

    def workspace_bytes(self) -> int:
        """The records of max_frames gather launches."""
        return int(lib.tdk_framestats_workspace_bytes(self.bins, self.channels, self.max_frames))

    def _check_frames(self, frames) -> list[torch.Tensor]:
        frames = [frames] if isinstance(frames, torch.Tensor) else list(frames)
        if not 1 <= len(frames) <= self.max_frames:
            raise ValueError(f'FrameStats takes 1..{self.max_frames} frames per call (max_frames), got {len(frames)}')
        shape = (self.height, self.width) if self.bayer_pattern is not None else (self.height, self.width, self.channels)
        for f in frames:
            if tuple(f.shape) != shape:
                raise RuntimeError(f'FrameStats input shape {tuple(f.shape)} != expected {shape}')
            _require(f.is_cuda, 'Input must be on CUDA device')
            _require(f.is_contiguous(), 'Input must be contiguous')
            _require(f.dtype in _TAGS, 'Input tensor must be float32, float16, uint8 or uint16')
            _require(f.dtype == frames[0].dtype and f.device == frames[0].device, 'The frames of a set must share their dtype and device')
        return frames

    def _run(self, frames) -> tuple[torch.Tensor, torch.Tensor]:
        """(counts, values): the two result blocks of the header."""
        frames = self._check_frames(frames)
        device, c, b, q = frames[0].device, self.channels, self.bins, len(self.quantiles)
        pointers = (ctypes.c_void_p * len(frames))(*(f.data_ptr() for f in frames))
        with torch.cuda.device(device):
            counts = torch.empty(c * (b + _COUNTERS), dtype=torch.int64, device=device)
            values = torch.empty(c + (c + 1) * q + 3, dtype=torch.float32, device=device)
            rc = lib.tdk_framestats(pointers, len(frames), _TAGS[frames[0].dtype], _ptr(self._workspace(device)), self.width, self.height, c,
                                    _pattern(self.bayer_pattern) if self.bayer_pattern is not None else 0, self.stride, b, self.lo, self.hi, self.min_count,
                                    self._c_quantiles if q else None, q, _ptr(counts), _ptr(values), _stream())
        check(rc)
        return counts, values

    def measure(self, frames) -> FrameStatistics:
        """A frame or a list of frames (at most max_frames, pooled) -> their statistics."""
        counts, values = self._run(frames)
        c, b, q = self.channels, self.bins, len(self.quantiles)
        table = counts.view(c, b + _COUNTERS)
        return FrameStatistics(hist=table[:, :b], below=table[:, b], above=table[:, b + 1], nan=table[:, b + 2], valid=table[:, b + 3], sum=table[:, b + 4],
                               mean=values[:c], percentiles=values[c:c + (c + 1) * q].view(c + 1, q), gains=values[c + (c + 1) * q:])

    def bounds(self, frames) -> torch.Tensor:
        """(2,) float32 on the device: the first and the last quantile of the pooled histogram -- the shape compute_image_bounds
        returns and normalize_image takes, but robust against a hot pixel, a specular highlight or a NaN."""
        if not self.quantiles:
            raise ValueError('bounds needs at least one quantile')
        _, values = self._run(frames)
        c, q = self.channels, len(self.quantiles)
        pooled = values[c + c * q:c + (c + 1) * q]
        return pooled if q == 2 else torch.stack((pooled[0], pooled[q - 1]))

    def white_balance(self, frames) -> torch.Tensor:
        """(3,) float32 grey-world gains (R, G, B) on the device, green = 1, each within [1/64, 64]; (1, 1, 1) when a channel has
        fewer than min_count valid values.  What apply_white_balance, Highlights.process and RCD.process_packed take."""
        if self.channels != 3:
            raise ValueError('white_balance needs three channels')
        _, values = self._run(frames)
        return values[-3:]


__all__ = ['FrameStats', 'FrameStatistics']
