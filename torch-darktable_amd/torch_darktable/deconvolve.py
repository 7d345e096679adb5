"""Capture sharpening (include/tdk_hip_deconv.h: tdk_deconv) -- Richardson-Lucy deconvolution of the luminance of a linear frame
with a small Gaussian PSF, held back by a contrast mask where the frame holds nothing but noise.

Lens, anti-alias filter and demosaic leave a blur; the unsharp mask in front of the encoder (Sharpen) raises edge contrast on
display-referred values and cannot undo it.  This stage runs on the linear frame straight after the demosaic:

    o      = max(luminance, 2^-20)
    u      = o;  N times:  u = u * G(o / G(u))            G: the separable blur with the PSF, the frame's edge replicated
    m      = smoothstep((sqrt(max3x3 o) - sqrt(min3x3 o) - threshold) / threshold)
    out_c  = x_c * clamp((o + m*(u - o)) / o, 1 / max_gain, max_gain)

The exact float32 formulas of the device are in the header, and a NumPy restatement (tests/deconv_spec.py) predicts the bits.  One
kernel runs `fused_iterations` iterations per launch inside LDS; u travels between the launches in float32 planes that belong to
the object, one set per stream.  No synchronisation: capturable in a HIP graph from the first call, and bit-reproducible.

    d = Deconvolve(device, (4096, 3072), sigma=0.7, iterations=8)
    sharp = d.process(rgb)                           # (H, W, 1 or 3) float32 or float16, the same type out; not clamped
    sharp, m = d.process(rgb, return_mask=True)      # m: (H, W) float32, where the stage acted
"""

from __future__ import annotations

import math

import torch

from ._frames import TAGS
from ._native import TDK_DECONV_FUSE_SHIFT, TDK_DECONV_MASK, TDK_DECONV_MAX_ITERATIONS, TDK_DECONV_MAX_RADIUS, TDK_DECONV_TILE, check, lib
from ._stage import FrameStage, SeparableTaps, as_float32, luma_weights
from .torch_darktable_extension import _ptr, _stream

MAX_GAIN = 16.0
BUILT_FUSED = {1: 6, 2: 4, 4: 2}   # F of an instantiation that was built: the largest radius it takes


class Deconvolve(FrameStage):
    """Deconvolve (H, W, 1 or 3) frames of one size (width, height).  sigma: the Gaussian PSF; iterations: N, 0 returns the input;
    threshold: the contrast, in the square-root domain, below which nothing is sharpened (None: no mask); max_gain: the largest
    factor a pixel is scaled by, up or down; weights: the luminance weights of three-channel frames."""

    TILE = (TDK_DECONV_TILE, TDK_DECONV_TILE)  # (width, height) of one workgroup's output tile (csrc/deconv.hip: DC_T)

    def __init__(self, device: torch.device, image_size: tuple[int, int], sigma: float = 0.7, iterations: int = 8, threshold: float | None = 0.02,
                 max_gain: float = 4.0, weights=None):
        taps = SeparableTaps.from_sigma(lib.tdk_deconv_weights, as_float32(sigma), 0.3, 2.0, TDK_DECONV_MAX_RADIUS)
        self._setup(device, image_size, taps, iterations, threshold, max_gain, weights)

    @staticmethod
    def from_weights(device: torch.device, image_size: tuple[int, int], taps, iterations: int = 8, threshold: float | None = 0.02, max_gain: float = 4.0,
                     weights=None) -> 'Deconvolve':
        """A caller's own symmetric PSF: taps (w0, w1, .. wR), 1 <= R <= 6, finite and >= 0, used as float32.  They are taken as
        they are; a PSF that keeps a flat area flat needs w0 + 2 (w1 + .. + wR) = 1."""
        self = Deconvolve.__new__(Deconvolve)
        self._setup(device, image_size, taps, iterations, threshold, max_gain, weights)
        return self

    def _setup(self, device, image_size, taps, iterations, threshold, max_gain, weights) -> None:
        super().__init__(device, image_size)
        self._taps = SeparableTaps.from_values(taps, TDK_DECONV_MAX_RADIUS, 'taps')
        self.sigma: float | None = self._taps.sigma
        if int(iterations) != iterations or not 0 <= int(iterations) <= TDK_DECONV_MAX_ITERATIONS:
            raise ValueError(f'iterations must be an integer in 0..{TDK_DECONV_MAX_ITERATIONS}, got {iterations}')
        if threshold is not None:
            threshold = as_float32(threshold)
            if not (math.isfinite(threshold) and threshold > 0.0):
                raise ValueError(f'threshold must be None or finite and > 0 as a float32, got {threshold}')
        max_gain = as_float32(max_gain)
        if not 1.0 <= max_gain <= MAX_GAIN:
            raise ValueError(f'max_gain must lie in [1, {MAX_GAIN:g}], got {max_gain}')
        self.weights, self._c_weights = luma_weights(weights)
        self.iterations, self.threshold, self.max_gain = int(iterations), threshold, max_gain
        self._forced = 0   # F forced through the flags (tests and measurements); 0: the library's choice
        self._prepare()

    @property
    def taps(self) -> tuple[float, ...]:
        """The PSF's taps w0 .. wR as float32 values."""
        return self._taps.values

    @property
    def radius(self) -> int:
        return self._taps.radius

    @property
    def fused_iterations(self) -> int:
        """F: the iterations one launch runs."""
        return self._forced or int(lib.tdk_deconv_fused_iterations(self.radius))

    @fused_iterations.setter
    def fused_iterations(self, fused: int | None) -> None:
        """Force F (every F gives the same bits: for tests and measurements); None: the library's choice."""
        fused = 0 if fused is None else int(fused)
        if fused != 0 and (fused not in BUILT_FUSED or self.radius > BUILT_FUSED[fused]):
            raise ValueError(f'fused_iterations must be None or one of {tuple(BUILT_FUSED)} that takes radius {self.radius} (radius <= {tuple(BUILT_FUSED.values())}), got {fused}')
        self._forced = fused

    @property
    def launches(self) -> int:
        return 1 if self.iterations == 0 else -(-self.iterations // self.fused_iterations)

    def _flags(self) -> int:
        return (TDK_DECONV_MASK if self.threshold is not None else 0) | (self._forced << TDK_DECONV_FUSE_SHIFT)

    def __repr__(self):
        threshold = None if self.threshold is None else f'{self.threshold:g}'
        return f'Deconvolve({self.width}x{self.height}, {self._taps!r}, radius={self.radius}, iterations={self.iterations}, threshold={threshold}, max_gain={self.max_gain:g})'

    def workspace_bytes(self) -> int:
        """Bytes of the planes u travels in between the launches; 0 when the call is one launch.  With a forced F: what any F needs."""
        if self._forced:
            return int(lib.tdk_deconv_workspace_bytes(self.width, self.height, TDK_DECONV_MAX_RADIUS, TDK_DECONV_MAX_ITERATIONS))
        return int(lib.tdk_deconv_workspace_bytes(self.width, self.height, self.radius, self.iterations))

    def lds_bytes(self, dtype: torch.dtype = torch.float32, channels: int = 3) -> int:
        """LDS one workgroup takes on frames of this kind (0: not a legal call)."""
        return int(lib.tdk_deconv_lds_bytes(channels, TAGS.get(dtype, -1), self.radius, self._flags()))

    def _run(self, image: torch.Tensor, want_mask: bool):
        height, width, channels, tag = self._float_frame(image, 'Deconvolve')
        with torch.cuda.device(image.device):
            out = torch.empty_like(image)
            m = torch.empty((height, width), dtype=torch.float32, device=image.device) if want_mask else None
            ws = self._workspace(image.device)
            rc = lib.tdk_deconv(_ptr(image), _ptr(out), _ptr(m), _ptr(ws if ws.numel() else None), width, height, channels, tag, self._taps.c_array, self.radius,
                                self.iterations, 1.0 if self.threshold is None else self.threshold, self.max_gain, self._c_weights, self._flags(), _stream())
        check(rc)
        return out, m

    def process(self, image: torch.Tensor, return_mask: bool = False):
        """(H, W, C) float32 or float16, C in {1, 3} -> the deconvolved frame of the same type, not clamped.  return_mask: (frame, m)
        with the (H, W) float32 contrast mask, 1 everywhere without a threshold."""
        out, m = self._run(image, bool(return_mask))
        return (out, m) if return_mask else out

    def mask(self, image: torch.Tensor) -> torch.Tensor:
        """The (H, W) float32 contrast mask alone (the frame is computed and dropped)."""
        return self._run(image, True)[1]


__all__ = ['Deconvolve']
