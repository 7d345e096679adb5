"""Noise profile (include/tdk_hip_noise.h) -- the block that measures how noisy a sensor is, and the transform that lets a denoiser
with one noise level serve a sensor whose noise grows with the signal.

Sensor noise is not one number: var(x) = a*x + b (shot noise plus read noise).  `NoiseProfile.estimate` fits a and b per colour on
raw mosaics: 8 x 8 blocks of every CFA plane give a mean and, from their second differences, a noise energy; the median energy per
intensity bin is a robust variance (texture only raises a minority of blocks), and a weighted line through the bins is the model.
`NoiseModel.stabilize` maps values so that the noise has the standard deviation sigma_out everywhere (the generalised Anscombe
transform), `NoiseModel.unstabilize` maps them back (the exact unbiased inverse of Makitalo and Foi, or the algebraic one):

    profile = NoiseProfile(device, (4096, 3072), BayerPattern.RGGB, white=1.0)
    model = profile.estimate(mosaic)                                   # device tensors; nothing is copied, nothing waits
    flat = model.stabilize(rgb, gains=white_balance, sigma_out=1.0)    # the noise of `flat` has sigma 1 in every channel
    w = Wavelet.from_sigma(device, (4096, 3072), (1.0, 1.0, 1.0))
    rgb = model.unstabilize(w.process(flat), gains=white_balance, out_dtype=rgb.dtype)

The exact formulas are in the header; a NumPy restatement (tests/noiseprofile_spec.py) predicts every integer and every float bit.
One gather launch for the whole set and two small finishing launches, or one streaming launch, on PyTorch's current stream; no
atomics on global memory, no memset, no copy, no synchronisation.  The workspace belongs to the object, one per stream, and is never
cleared: capturable in a HIP graph from the first call, and bit-reproducible.

The profile is measured on the raw mosaic, where the noise of neighbouring sites is independent.  A demosaic interpolates and so
correlates the noise of an RGB frame and lowers its variance a little: on RGB the raw-domain profile (with the white-balance gains)
is an approximation.  darktable makes the same one.  The intercept b is an extrapolation when shot noise dominates the darkest bin
that has enough blocks: it comes out low there (0.58 .. 0.98 of the truth on the synthetic chart of tests/test_noiseprofile_spec.py)
while a stays within a few percent.  Fusing the transform into the loads and stores of the denoisers is the follow-up.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from ._frames import MAX_SIZE
from ._mosaic import FLOAT_TAGS, MosaicStage, check_gains, check_pattern, check_storage, out_dtype_of
from ._native import (TDK_F16, TDK_F32, TDK_NOISE_ALGEBRAIC, TDK_NOISE_GRID, TDK_NOISE_LEVELS, TDK_NOISE_MAX_BINS, TDK_NOISE_MAX_FRAMES, TDK_NOISE_STRIP_BYTES,
                      TDK_NOISE_UNBIASED, TDK_U16, check, lib)
from ._stage import as_float32 as _f32
from .bayer import BayerPattern
from .torch_darktable_extension import _pattern, _ptr, _require, _stream

_TAGS = {torch.float32: TDK_F32, torch.float16: TDK_F16, torch.uint16: TDK_U16}
_INVERSES = {'algebraic': TDK_NOISE_ALGEBRAIC, 'unbiased': TDK_NOISE_UNBIASED}
_COUNTERS = 9  # all, nan, clipped per colour


@dataclass
class NoiseStatistics:
    """What `NoiseProfile.statistics` returns: the integer block, every tensor int64 on the device.  I bins, 128 levels."""

    hist: torch.Tensor      # (3, I, 128): valid blocks per colour, intensity bin and energy level
    sum: torch.Tensor       # (3, I): the sum of q over their samples
    blocks: torch.Tensor    # (3,): all complete blocks
    nan: torch.Tensor       # (3,): blocks with a NaN
    clipped: torch.Tensor   # (3,): blocks without a NaN that reach below clip_lo or above clip_hi


class NoiseModel:
    """var(x) = a*x + b per colour (R, G, B).  model: (3, 4) float32 rows of a, b, valid, usable bins; curve: (2, 3, I) float32, the
    mean and the variance of every intensity bin (0 where the bin was not usable), for a display.  Both stay where they were made."""

    def __init__(self, model: torch.Tensor, curve: torch.Tensor | None = None):
        if tuple(model.shape) != (3, 4) or model.dtype != torch.float32 or not model.is_contiguous():
            raise ValueError(f'model must be a contiguous (3, 4) float32 tensor, got {tuple(model.shape)} {model.dtype}')
        if curve is not None and (curve.dim() != 3 or tuple(curve.shape[:2]) != (2, 3) or curve.dtype != torch.float32):
            raise ValueError(f'curve must be a (2, 3, bins) float32 tensor, got {tuple(curve.shape)} {curve.dtype}')
        self.model, self.curve = model, curve

    @property
    def a(self) -> torch.Tensor:
        return self.model[:, 0]

    @property
    def b(self) -> torch.Tensor:
        return self.model[:, 1]

    @property
    def valid(self) -> torch.Tensor:
        return self.model[:, 2]

    def __repr__(self):
        return f'NoiseModel(device={self.model.device}, bins={None if self.curve is None else self.curve.shape[2]})'

    @staticmethod
    def _three(values, what: str) -> tuple[float, float, float]:
        if isinstance(values, torch.Tensor):
            values = values.tolist()
        values = (float(values),) * 3 if isinstance(values, (int, float)) else tuple(float(v) for v in values)
        if len(values) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in values):
            raise ValueError(f'{what} must be one or three finite values >= 0, got {values}')
        return values

    @staticmethod
    def from_values(a, b, device: torch.device) -> 'NoiseModel':
        """A known model: a and b are one value or three (R, G, B), finite and >= 0.  Every row is valid."""
        a, b = NoiseModel._three(a, 'a'), NoiseModel._three(b, 'b')
        return NoiseModel(torch.tensor([[a[k], b[k], 1.0, 0.0] for k in range(3)], dtype=torch.float32, device=device))

    def to_dict(self) -> dict:
        """Host side, for a camera settings JSON: copies the twelve numbers and waits for them."""
        rows = self.model.detach().cpu().tolist()
        return {'a': [r[0] for r in rows], 'b': [r[1] for r in rows], 'valid': [bool(r[2]) for r in rows], 'bins': [int(r[3]) for r in rows]}

    @staticmethod
    def from_dict(values: dict, device: torch.device) -> 'NoiseModel':
        a, b = NoiseModel._three(values['a'], 'a'), NoiseModel._three(values['b'], 'b')
        valid, bins = values.get('valid', (True,) * 3), values.get('bins', (0,) * 3)
        if len(tuple(valid)) != 3 or len(tuple(bins)) != 3:
            raise ValueError('valid and bins must hold three values')
        return NoiseModel(torch.tensor([[a[k], b[k], 1.0 if valid[k] else 0.0, float(bins[k])] for k in range(3)], dtype=torch.float32, device=device))

    def _transform(self, forward: bool, x: torch.Tensor, bayer_pattern, gains, sigma_out, inverse, out_dtype) -> torch.Tensor:
        what = 'stabilize' if forward else 'unstabilize'
        if bayer_pattern is not None:
            check_pattern(bayer_pattern)
            if x.dim() != 2 or x.shape[0] % 2 or x.shape[1] % 2 or not (2 <= x.shape[0] <= MAX_SIZE and 2 <= x.shape[1] <= MAX_SIZE):
                raise ValueError(f'{what}: a mosaic is (H, W) with H and W even, 2..{MAX_SIZE}, got {tuple(x.shape)}')
            channels, width = 1, int(x.shape[1])
        else:
            if x.dim() < 1 or x.shape[-1] not in (1, 3):
                raise ValueError(f'{what}: an image is (..., C) with C = 1 or 3, got {tuple(x.shape)}')
            channels, width = int(x.shape[-1]), 0
        if x.numel() == 0:
            raise ValueError(f'{what}: empty input')
        sigma_out = _f32(sigma_out)
        if not (math.isfinite(sigma_out) and sigma_out > 0.0):
            raise ValueError(f'sigma_out must be finite and > 0, got {sigma_out}')
        if inverse not in _INVERSES:
            raise ValueError(f"inverse must be 'unbiased' or 'algebraic', got {inverse!r}")
        out_dtype = out_dtype_of(out_dtype, x.dtype)
        check_storage(x)
        _require(self.model.device == x.device, 'The model must be on the device of the input')
        check_gains(gains, x.device)
        pattern = _pattern(bayer_pattern) if bayer_pattern is not None else 0
        with torch.cuda.device(x.device):
            out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
            if forward:
                rc = lib.tdk_noise_stabilize(_ptr(x), FLOAT_TAGS[x.dtype], _ptr(out), FLOAT_TAGS[out_dtype], x.numel(), width, channels, pattern, _ptr(self.model),
                                             _ptr(gains), sigma_out, _stream())
            else:
                rc = lib.tdk_noise_unstabilize(_ptr(x), FLOAT_TAGS[x.dtype], _ptr(out), FLOAT_TAGS[out_dtype], x.numel(), width, channels, pattern, _ptr(self.model),
                                               _ptr(gains), sigma_out, _INVERSES[inverse], _stream())
        check(rc)
        return out

    def stabilize(self, x: torch.Tensor, bayer_pattern: BayerPattern | None = None, gains: torch.Tensor | None = None, sigma_out: float = 1.0,
                  out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """x -> y whose noise has the standard deviation sigma_out.  x is an (H, W) mosaic (bayer_pattern given: the colour of a site
        picks the model row) or a (..., C) image, C = 3 (row = channel) or 1 (row 0), float32 or float16.  gains: a (3,) float32 device
        tensor, the white-balance gains x has been multiplied by since the model was measured."""
        return self._transform(True, x, bayer_pattern, gains, sigma_out, 'unbiased', out_dtype)

    def unstabilize(self, y: torch.Tensor, bayer_pattern: BayerPattern | None = None, gains: torch.Tensor | None = None, sigma_out: float = 1.0,
                    inverse: str = 'unbiased', out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """The way back, with the arguments `stabilize` was given.  inverse='unbiased': the mean of the result is the mean of the signal
        (what a denoised frame needs); 'algebraic': the exact inverse function.  out_dtype None: the type of y."""
        return self._transform(False, y, bayer_pattern, gains, sigma_out, inverse, out_dtype)


def _set_noise_model(stage, model: NoiseModel) -> None:
    if not isinstance(model, NoiseModel):
        raise TypeError(f'noise_model must be a NoiseModel, got {type(model).__name__}')
    stage._noise_model = model


# the `noise_model` of TemporalDenoise and HdrMerge: any NoiseModel, exchangeable between calls
NOISE_MODEL = property(lambda stage: stage._noise_model, _set_noise_model)


class NoiseProfile(MosaicStage):
    """Measure the noise model of mosaics of one size; image_size is (width, height), both even.  `white` is the value of a saturated
    site (1.0 for normalised frames, 65535 for uint16 taken as it is); `clip` = (clip_lo, clip_hi) are the limits, in 16-bit units of
    white, outside which a block is left out (black clipping folds the noise, saturation removes it)."""

    GRID = TDK_NOISE_GRID                  # workgroups of the gather launch, whatever the frame size (csrc/noiseprofile.hip: NP_GRID)
    STRIP_BYTES = TDK_NOISE_STRIP_BYTES    # bytes of each of 16 rows a workgroup takes per step
    LEVELS = TDK_NOISE_LEVELS

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, bins: int = 32, white: float = 1.0,
                 clip: tuple[int, int] = (1, 64224), min_count: int = 32, max_frames: int = 1):
        super().__init__(device, image_size)
        check_pattern(bayer_pattern)
        self._check_even()
        if int(bins) != bins or not 2 <= int(bins) <= TDK_NOISE_MAX_BINS:
            raise ValueError(f'bins must be an integer in 2..{TDK_NOISE_MAX_BINS}, got {bins}')
        white = _f32(white)
        if not (math.isfinite(white) and white > 0.0 and math.isfinite(_f32(65535.0 / white))):
            raise ValueError(f'white must be finite and > 0, got {white}')
        if len(tuple(clip)) != 2 or any(int(v) != v for v in clip) or not 0 <= int(clip[0]) <= int(clip[1]) <= 65535:
            raise ValueError(f'clip must be integers (clip_lo, clip_hi) with 0 <= clip_lo <= clip_hi <= 65535, got {tuple(clip)}')
        if int(min_count) != min_count or not 1 <= int(min_count) < 2 ** 31:
            raise ValueError(f'min_count must be an integer >= 1, got {min_count}')
        if int(max_frames) != max_frames or not 1 <= int(max_frames) <= TDK_NOISE_MAX_FRAMES:
            raise ValueError(f'max_frames must be an integer in 1..{TDK_NOISE_MAX_FRAMES}, got {max_frames}')
        self.bayer_pattern = bayer_pattern
        self.bins, self.white, self.clip = int(bins), white, (int(clip[0]), int(clip[1]))
        self.min_count, self.max_frames = int(min_count), int(max_frames)
        self._keep_workspace()

    def __repr__(self):
        return (f'NoiseProfile({self.width}x{self.height}, {self.bayer_pattern.name}, bins={self.bins}, white={self.white:g}, clip={self.clip}, '
                f'min_count={self.min_count}, max_frames={self.max_frames})')

    def lds_bytes(self) -> int:
        """LDS of a workgroup of the gather launch: the level histograms, the sums, the counters and the staged strip."""
        return int(lib.tdk_noise_lds_bytes(self.bins))

    def workspace_bytes(self) -> int:
        """The records of the gather launch; the number of frames does not enter."""
        return int(lib.tdk_noise_workspace_bytes(self.bins))

    def _check_frames(self, mosaics) -> list[torch.Tensor]:
        frames = [mosaics] if isinstance(mosaics, torch.Tensor) else list(mosaics)
        if not 1 <= len(frames) <= self.max_frames:
            raise ValueError(f'NoiseProfile takes 1..{self.max_frames} frames per call (max_frames), got {len(frames)}')
        for f in frames:
            self._check_mosaic(f, 'input', _TAGS, 'float32, float16 or uint16')
            _require(f.dtype == frames[0].dtype and f.device == frames[0].device, 'The frames of a set must share their dtype and device')
        return frames

    def _run(self, mosaics) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(counts, model, curve): the three result blocks of the header."""
        frames = self._check_frames(mosaics)
        device, bins = frames[0].device, self.bins
        pointers = (ctypes.c_void_p * len(frames))(*(f.data_ptr() for f in frames))
        with torch.cuda.device(device):
            counts = torch.empty(3 * bins * TDK_NOISE_LEVELS + 3 * bins + _COUNTERS, dtype=torch.int64, device=device)
            model = torch.empty((3, 4), dtype=torch.float32, device=device)
            curve = torch.empty((2, 3, bins), dtype=torch.float32, device=device)
            rc = lib.tdk_noise_profile(pointers, len(frames), _TAGS[frames[0].dtype], _ptr(self._workspace(device)), self.width, self.height,
                                       _pattern(self.bayer_pattern), bins, self.white, self.clip[0], self.clip[1], self.min_count, _ptr(counts), _ptr(model),
                                       _ptr(curve), _stream())
        check(rc)
        return counts, model, curve

    def estimate(self, mosaics) -> NoiseModel:
        """A mosaic or a list of mosaics (at most max_frames, pooled) -> their noise model."""
        _, model, curve = self._run(mosaics)
        return NoiseModel(model, curve)

    def statistics(self, mosaics) -> NoiseStatistics:
        """The integer block the model is derived from."""
        counts, _, _ = self._run(mosaics)
        bins, words = self.bins, 3 * self.bins * TDK_NOISE_LEVELS
        tail = counts[words + 3 * bins:].view(3, 3)
        return NoiseStatistics(hist=counts[:words].view(3, bins, TDK_NOISE_LEVELS), sum=counts[words:words + 3 * bins].view(3, bins), blocks=tail[0], nan=tail[1],
                               clipped=tail[2])


__all__ = ['NoiseProfile', 'NoiseModel', 'NoiseStatistics']
