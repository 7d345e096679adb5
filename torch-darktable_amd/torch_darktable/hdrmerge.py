"""Exposure-bracket merge (include/tdk_hip_hdr.h) -- 2 to 8 raw Bayer mosaics of one scene at different exposures become one mosaic.

A scene with more range than the sensor is shot as a bracket.  `HdrMerge` combines the frames per site by inverse-variance weights from
the noise model var(x) = a*x + b: the result has the highlights of the shortest exposure and the shadow noise of the longest.  A frame
that is clipped at a site (or next to it) has no weight there; a frame that disagrees with the site's anchor frame -- the longest
unclipped one by default -- beyond what the model predicts loses its weight by the window statistic of `TemporalDenoise`, so that what
moved between the exposures leaves no ghost.

    profile = NoiseProfile(device, (4096, 3072), BayerPattern.RGGB)
    merge = HdrMerge(device, (4096, 3072), BayerPattern.RGGB, profile.estimate(mosaic))
    hdr = merge.process([long, mid, short], exposures=(1 / 30, 1 / 120, 1 / 480))   # radiance in the units of the shortest frame

It acts on raw mosaics only, in front of the white balance and the demosaic: there the noise of neighbouring sites is independent and
the model is exact.  The result lies in the range one frame has, so the white balance, `Highlights` and the bounds downstream see
what they expect; a noise model of the merged mosaic is not provided.  The exact formulas are in the header; a NumPy restatement
(tests/hdrmerge_spec.py) predicts every bit of the output and every byte of the mask.  One tile launch on PyTorch's current stream; no
workspace, no atomics, no memset, no copy, no synchronisation.  The exposures and the twelve numbers of the noise model are read from
device memory by every call: an auto-exposure or a `NoiseProfile.estimate` earlier on the stream feeds a captured merge.
"""

from __future__ import annotations

import ctypes
import math

import torch

from ._mosaic import FLOAT_TAGS, MosaicStage, check_frame_set, check_pattern, check_radius, out_dtype_of, positive_float32, window_repr, window_thresholds
from ._native import TDK_HDR_MAX_FRAMES, TDK_HDR_TILE_H, TDK_HDR_TILE_W, check, lib
from ._stage import as_float32 as _f32
from ._streams import StreamBuffers
from .bayer import BayerPattern
from .noiseprofile import NOISE_MODEL, NoiseModel
from .torch_darktable_extension import _pattern, _ptr, _require, _stream


class HdrMerge(MosaicStage):
    """Merge of brackets of (H, W) mosaics of one size; image_size is (width, height), both even.  `clip`: a sample at or above it is
    clipped, and so are its eight neighbours.  `thresholds`, `pixel_threshold`, `radius` and `variance_floor` are those of
    `TemporalDenoise`: it is the same statistic, between a frame and the anchor frame of a site."""

    TILE = (TDK_HDR_TILE_W, TDK_HDR_TILE_H)   # the output tile of a workgroup (csrc/hdrmerge.hip)
    MAX_FRAMES = TDK_HDR_MAX_FRAMES

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, noise_model: NoiseModel, radius: int = 2,
                 clip: float = 0.95, thresholds: tuple[float, float] = (1.5, 3.0), pixel_threshold: float | None = 4.0, variance_floor: float = 1e-12):
        super().__init__(device, image_size)
        check_pattern(bayer_pattern)
        self._check_even()
        check_radius(radius)
        self.clip = positive_float32(clip, 'clip')
        self.thresholds, self.pixel_threshold, self._c2 = window_thresholds(thresholds, pixel_threshold)
        self.variance_floor = positive_float32(variance_floor, 'variance_floor')
        self.bayer_pattern, self.radius = bayer_pattern, int(radius)
        self.noise_model = noise_model
        self._exposures = StreamBuffers()   # one uploaded copy per distinct tuple of floats and stream

    noise_model = NOISE_MODEL

    def __repr__(self):
        return (f'HdrMerge({self.width}x{self.height}, {self.bayer_pattern.name}, radius={self.radius}, clip={self.clip:g}, {window_repr(self)})')

    def lds_bytes(self) -> int:
        """Static LDS of a workgroup: the staged planes, the row sums, the clip bits and the table of frames."""
        return int(lib.tdk_hdr_lds_bytes(self.radius))

    def _frames(self, frames) -> list[torch.Tensor]:
        if isinstance(frames, torch.Tensor):
            if frames.ndim != 3:
                raise RuntimeError(f'HdrMerge input shape {tuple(frames.shape)}: a stacked bracket is (F, H, W)')
            frames = list(frames.unbind(0))
        frames = list(frames)
        if not 2 <= len(frames) <= TDK_HDR_MAX_FRAMES:
            raise ValueError(f'a bracket has 2..{TDK_HDR_MAX_FRAMES} frames, got {len(frames)}')
        shape = (self.height, self.width)
        for f, frame in enumerate(frames):
            if not isinstance(frame, torch.Tensor) or tuple(frame.shape) != shape:
                raise RuntimeError(f'HdrMerge input shape {tuple(getattr(frame, "shape", ()))} of frame {f} != expected {shape}')
        return frames

    @staticmethod
    def _exposure_values(exposures, count: int):
        """The exposures as the host holds them: a device tensor as it is (nothing of it is checked), floats as a checked tuple."""
        if isinstance(exposures, torch.Tensor):
            _require(tuple(exposures.shape) == (count,) and exposures.dtype == torch.float32 and exposures.is_contiguous(),
                     f'exposures must be a contiguous ({count},) float32 tensor')
            return exposures
        values = tuple(_f32(v) for v in exposures)
        if len(values) != count:
            raise ValueError(f'{count} frames need {count} exposures, got {len(values)}')
        if not all(math.isfinite(v) and v > 0.0 for v in values):
            raise ValueError(f'exposures must be finite and > 0 as float32, got {tuple(exposures)}')
        return values

    def _exposure_tensor(self, exposures, device: torch.device) -> torch.Tensor:
        if isinstance(exposures, torch.Tensor):
            _require(exposures.device == device, 'exposures must be on the device of the frames')
            return exposures
        known = len(self._exposures)
        buf = self._exposures.get(4 * len(exposures), device, key=exposures).view(torch.float32)
        if len(self._exposures) != known:   # a tuple first seen on this stream: the one upload (not inside a capture)
            buf.copy_(torch.tensor(exposures, dtype=torch.float32))
        return buf

    def _arguments(self, frames, exposures, ref, out_dtype):
        """The checks of `process`: (frames as a list, the exposures as the host holds them, out_dtype, the model tensor)."""
        frames = self._frames(frames)
        count = len(frames)
        first = frames[0]
        out_dtype = out_dtype_of(out_dtype, first.dtype)
        if ref is not None and (isinstance(ref, bool) or int(ref) != ref or not 0 <= ref < count):
            raise ValueError(f'ref must be None or a frame index below {count}, got {ref}')
        exposures = self._exposure_values(exposures, count)
        check_frame_set(frames)
        model = self._noise_model.model
        _require(model.device == first.device, 'The model must be on the device of the input')
        return frames, exposures, out_dtype, model

    def process(self, frames, exposures, ref: int | None = None, out_dtype: torch.dtype | None = None, return_mask: bool = False):
        """A bracket -> the merged mosaic, a fresh tensor; with return_mask also the (H, W) uint8 mask: the anchor frame in bits 0..2, 8
        where every frame is clipped, the number of frames with weight in bits 4..7.  frames: a list of (H, W) tensors or one (F, H, W)
        tensor, all float32 or all float16, each contiguous.  exposures: F floats (finite and > 0; uploaded once per distinct tuple and
        stream) or a device tensor of F floats, read by the kernel and not checked.  ref: the anchor frame of the sites it does not clip;
        None: the longest exposure."""
        frames, exposures, out_dtype, model = self._arguments(frames, exposures, ref, out_dtype)
        count, first = len(frames), frames[0]
        shape = (self.height, self.width)
        with torch.cuda.device(first.device):
            exp = self._exposure_tensor(exposures, first.device)
            out = torch.empty(shape, dtype=out_dtype, device=first.device)
            mask = torch.empty(shape, dtype=torch.uint8, device=first.device) if return_mask else None
            pointers = (ctypes.c_void_p * count)(*[frame.data_ptr() for frame in frames])
            rc = lib.tdk_hdr_merge(pointers, count, FLOAT_TAGS[first.dtype], _ptr(out), FLOAT_TAGS[out_dtype], _ptr(mask), self.width, self.height,
                                   _pattern(self.bayer_pattern), _ptr(exp), -1 if ref is None else int(ref), _ptr(model), self.radius, self.clip,
                                   self.thresholds[0], self.thresholds[1], self._c2, self.variance_floor, _stream())
        check(rc)
        return (out, mask) if return_mask else out


__all__ = ['HdrMerge']
