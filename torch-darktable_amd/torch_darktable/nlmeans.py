"""Non-local means denoiser (include/tdk_hip_denoise.h: tdk_nlmeans) -- the spatial-domain companion of `denoise.Wiener`.

Every output pixel is the average of the pixels of its (2S+1)^2 search window, weighted by exp(-D / h^2), D the mean squared
difference (channel-weighted) of the (2P+1)^2 patches around the two pixels.  Patch samples beyond the frame replicate the
edge; candidates beyond the frame are skipped.  One kernel launch on PyTorch's current stream, no workspace, no
synchronisation: capturable in a HIP graph from the first call, and bit-reproducible.

    nlm = NLMeans(device, (width, height))            # S = 7, P = 2
    out = nlm.process(image, h=0.1)                   # (H, W, 1 or 3), float32 or float16 storage
    out = nlm.process_log_luminance(rgb, h=0.1)       # lightness only: texture-preserving luminance denoising
    out = nlm.process(rgb, 0.1, channel_weights=(1.0, 0.25, 0.25))
"""

from __future__ import annotations

import ctypes
import math

import torch

from ._native import check, lib
from .extension import extension
from .torch_darktable_extension import _dtype_tag, _ptr, _require, _stream

MAX_SEARCH_RADIUS, MAX_PATCH_RADIUS = 10, 4


class NLMeans:
    """Non-local means for a fixed image size: search radius 1..10, patch radius 1..4."""

    def __init__(self, device: torch.device, image_size: tuple[int, int], search_radius: int = 7, patch_radius: int = 2):
        width, height = image_size
        if device.type != 'cuda':
            raise ValueError(f'Device must be CUDA, got {device}')
        if width <= 0 or height <= 0:
            raise ValueError(f'Image dimensions must be positive, got {width}x{height}')
        if not 1 <= search_radius <= MAX_SEARCH_RADIUS:
            raise ValueError(f'search_radius must be 1..{MAX_SEARCH_RADIUS}, got {search_radius}')
        if not 1 <= patch_radius <= MAX_PATCH_RADIUS:
            raise ValueError(f'patch_radius must be 1..{MAX_PATCH_RADIUS}, got {patch_radius}')
        self._device = device
        self.width, self.height = int(width), int(height)
        self.search_radius, self.patch_radius = int(search_radius), int(patch_radius)

    def __repr__(self):
        return f'NLMeans({self.width}x{self.height}, search_radius={self.search_radius}, patch_radius={self.patch_radius})'

    def process(self, image: torch.Tensor, h: float, channel_weights=None) -> torch.Tensor:
        """Denoise an (H, W, C) image, C in {1, 3}.  h: the filter strength (about the noise sigma times 2..4);
        channel_weights: C non-negative floats weighting the channels in the patch distance (default all 1)."""
        assert image.dim() == 3, f'image must have 3 dimensions, got {image.shape}'
        expected = (self.height, self.width, image.size(2))
        if tuple(image.shape) != expected:
            raise RuntimeError(f'NLMeans input shape {tuple(image.shape)} != expected {expected}')
        channels = image.size(2)
        if channels not in {1, 3}:
            raise ValueError(f'image channels must be 1 or 3, got {channels}')
        h = float(h)
        if not (math.isfinite(h) and h > 0.0):
            raise ValueError(f'h must be positive and finite, got {h}')
        weights = None
        if channel_weights is not None:
            values = [float(v) for v in channel_weights]
            if len(values) != channels:
                raise ValueError(f'channel_weights must have {channels} elements for {channels}-channel image')
            if any(not math.isfinite(v) or v < 0.0 for v in values) or not any(v > 0.0 for v in values):
                raise ValueError(f'channel_weights must be finite, not negative and not all zero, got {values}')
            weights = (ctypes.c_float * channels)(*values)
        _require(image.is_cuda, 'Input must be on CUDA device')
        _require(image.is_contiguous(), 'Input must be contiguous')
        tag = _dtype_tag(image)
        with torch.cuda.device(image.device):
            out = torch.empty_like(image)
            rc = lib.tdk_nlmeans(_ptr(image), _ptr(out), self.width, self.height, channels, tag, self.search_radius, self.patch_radius, h,
                                 ctypes.cast(weights, ctypes.c_void_p) if weights is not None else None, _stream())
        check(rc)
        return out

    def process_luminance(self, image: torch.Tensor, h: float) -> torch.Tensor:
        """Denoise the Lab lightness of an RGB image and keep a/b (extract -> process -> replace)."""
        lum = extension.compute_luminance(image)
        return extension.modify_luminance(image, self.process(lum.unsqueeze(2), h).squeeze(2))

    def process_log_luminance(self, image: torch.Tensor, h: float, eps: float = 1e-4) -> torch.Tensor:
        """process_luminance on log(max(eps, lightness))."""
        lum = extension.compute_log_luminance(image, eps)
        return extension.modify_log_luminance(image, self.process(lum.unsqueeze(2), h).squeeze(2), eps)


__all__ = ['NLMeans']
