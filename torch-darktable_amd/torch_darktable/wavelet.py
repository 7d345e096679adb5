"""Wavelet-shrinkage denoiser (include/tdk_hip_wavelet.h: tdk_wavelet) -- the multi-scale companion of `denoise.Wiener` and
`nlmeans.NLMeans`, with a luma/chroma mode for the colour noise a demosaic leaves.

The frame is split into `scales` detail bands by the a-trous B3-spline filter (taps 1 4 6 4 1 / 16 at steps 1, 2, 4, ..., the frame's
edge replicated at every scale); every detail coefficient is shrunk towards zero by the threshold of its band and channel, and the
bands are added back to the coarsest approximation.  With `ycc` an RGB frame is processed as Y = (R + 2G + B) / 4, Cb = B - G,
Cr = R - G, so that the chroma planes can be denoised harder than the luma.  At most max(1, scales - 1) kernel launches on
PyTorch's current stream, no synchronisation; the workspace belongs to the object, one per stream: capturable in a HIP graph from
the first call, and bit-reproducible.

    w = Wavelet(device, (width, height), scales=4, thresholds=0.01)             # (H, W, 1 or 3); float32 or float16
    w = Wavelet.from_sigma(device, (width, height), estimate_channel_noise(rgb))   # thresholds from a noise estimate, luma/chroma
    out = w.process(rgb)
"""

from __future__ import annotations

import ctypes
import math

import torch

from ._frames import TAGS, check_frame, check_size, require_cuda_device
from ._native import TDK_WAVELET_MAX_SCALES, TDK_WAVELET_YCC, check, lib
from ._stage import as_float32 as _f32
from ._streams import StreamBuffers
from .extension import extension
from .torch_darktable_extension import _ptr, _stream


def band_norms(scales: int) -> tuple[float, ...]:
    """n_s, s = 0 .. scales - 1: the standard deviation white noise of sigma 1 leaves in detail band s (float32 values)."""
    buf = (ctypes.c_float * TDK_WAVELET_MAX_SCALES)()
    if lib.tdk_wavelet_band_norms(int(scales), buf) != 0:
        raise ValueError(lib.tdk_last_error().decode('utf-8', 'replace'))
    return tuple(buf[: int(scales)])


class Wavelet:
    """A-trous wavelet shrinkage for a fixed image size (width, height).  thresholds: one value, `scales` values (one per band, finest
    first) or `scales` rows of `channels` values; a flat list fixes no channel count and serves frames of 1 and of 3 channels.  With
    `ycc` the channels of a row are Y, Cb, Cr and the frames must have three channels."""

    TILE = (32, 32)  # (width, height) of one workgroup's output tile in the fine launch (csrc/wavelet.hip: WV_TW, WV_TH)
    FUSED = 2        # the scales the fine launch fuses (WV_FUSED): up to here one launch and no workspace

    def __init__(self, device: torch.device, image_size: tuple[int, int], scales: int = 4, thresholds=0.0, ycc: bool = False):
        require_cuda_device(device)
        check_size('Image', image_size)
        scales = int(scales)
        if not 1 <= scales <= TDK_WAVELET_MAX_SCALES:
            raise ValueError(f'scales must be 1..{TDK_WAVELET_MAX_SCALES}, got {scales}')
        self._device = device
        self.width, self.height = int(image_size[0]), int(image_size[1])
        self.scales, self.ycc = scales, bool(ycc)
        self._rows, self.channels = self._threshold_rows(thresholds, scales)
        if self.ycc and self.channels == 1:
            raise ValueError('ycc needs three channels, the thresholds have one per scale')
        self._c_thresholds: dict[int, ctypes.Array] = {}
        self._workspaces = StreamBuffers()
        if torch.cuda.is_available():   # (an object can be built and queried without a GPU; nothing runs there)
            self._workspace(torch.device('cuda', torch.cuda.current_device()) if device.index is None else device)

    @staticmethod
    def _threshold_rows(thresholds, scales: int) -> tuple[tuple[tuple[float, ...], ...], int | None]:
        """(a row of thresholds per scale, the channel count they fix or None)."""
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.tolist()
        if isinstance(thresholds, (int, float)):
            rows, channels = tuple((_f32(thresholds),) for _ in range(scales)), None
        else:
            values = list(thresholds)
            if len(values) != scales:
                raise ValueError(f'thresholds must be one value, {scales} values or {scales} rows of values, got {len(values)}')
            if all(isinstance(v, (int, float)) for v in values):
                rows, channels = tuple((_f32(v),) for v in values), None
            else:
                rows = tuple(tuple(_f32(v) for v in row) for row in values)
                channels = len(rows[0])
                if channels not in {1, 3} or any(len(row) != channels for row in rows):
                    raise ValueError(f'threshold rows must all hold 1 or all hold 3 values, got {[len(row) for row in rows]}')
        if not all(math.isfinite(v) and v >= 0.0 for row in rows for v in row):
            raise ValueError(f'thresholds must be finite and >= 0, got {rows}')
        return rows, channels

    @staticmethod
    def from_sigma(device: torch.device, image_size: tuple[int, int], sigma, scales: int = 4, strength: float = 3.0, ycc: bool = True) -> 'Wavelet':
        """Thresholds from the noise of the RGB channels (three values, say denoise.estimate_channel_noise(rgb)):
        t[s][k] = strength * sigma_k * n_s, n_s the noise gain of band s.  With ycc, sigma_k is the noise the transform leaves in Y, Cb, Cr."""
        if isinstance(sigma, torch.Tensor):
            sigma = sigma.tolist()
        sr, sg, sb = (float(v) for v in sigma)
        if not all(math.isfinite(v) and v >= 0.0 for v in (sr, sg, sb)):
            raise ValueError(f'sigma must be finite and >= 0, got {(sr, sg, sb)}')
        strength = float(strength)
        if not (math.isfinite(strength) and strength >= 0.0):
            raise ValueError(f'strength must be finite and >= 0, got {strength}')
        if ycc:
            per = (math.sqrt(sr * sr + 4.0 * sg * sg + sb * sb) / 4.0, math.sqrt(sb * sb + sg * sg), math.sqrt(sr * sr + sg * sg))
        else:
            per = (sr, sg, sb)
        scales = int(scales)
        if not 1 <= scales <= TDK_WAVELET_MAX_SCALES:
            raise ValueError(f'scales must be 1..{TDK_WAVELET_MAX_SCALES}, got {scales}')
        rows = [[strength * s * n for s in per] for n in band_norms(scales)]
        return Wavelet(device, image_size, scales, rows, ycc)

    @property
    def thresholds(self) -> tuple[tuple[float, ...], ...]:
        """A row per scale, finest first, as float32 values: one value for every channel, or one per channel."""
        return self._rows

    def __repr__(self):
        return f'Wavelet({self.width}x{self.height}, scales={self.scales}, ycc={self.ycc}, thresholds={self._rows})'

    def _flags(self) -> int:
        return TDK_WAVELET_YCC if self.ycc else 0

    def lds_bytes(self, channels: int, dtype: torch.dtype) -> int:
        """The largest LDS use of a workgroup on frames of this kind (0: not a legal call)."""
        return int(lib.tdk_wavelet_lds_bytes(channels, TAGS.get(dtype, -1), self.scales, self._flags()))

    def workspace_bytes(self, channels: int = 3) -> int:
        return int(lib.tdk_wavelet_workspace_bytes(self.width, self.height, channels, self.scales))

    def _workspace(self, device: torch.device) -> torch.Tensor | None:
        """The float32 planes between the launches, one buffer per stream (sized for three channels): the object may be used from
        several streams at once.  The buffer of the stream current at construction exists from then on, so a capture allocates nothing."""
        nbytes = self.workspace_bytes(3)
        return self._workspaces.get(nbytes, device) if nbytes else None

    def _threshold_array(self, channels: int) -> ctypes.Array:
        arr = self._c_thresholds.get(channels)
        if arr is None:
            flat = [row[k if len(row) > 1 else 0] for row in self._rows for k in range(channels)]
            arr = self._c_thresholds[channels] = (ctypes.c_float * len(flat))(*flat)
        return arr

    def process(self, image: torch.Tensor) -> torch.Tensor:
        """(H, W, C) -> (H, W, C), C in {1, 3}, float32 or float16, the same type out."""
        height, width, channels, tag = check_frame(image, (self.height, self.width), 'Wavelet')
        if self.channels is not None and channels != self.channels:
            raise ValueError(f'image channels must be {self.channels} (the thresholds are per channel), got {channels}')
        if self.ycc and channels != 3:
            raise ValueError(f'image channels must be 3 with ycc, got {channels}')
        with torch.cuda.device(image.device):
            out = torch.empty_like(image)
            rc = lib.tdk_wavelet(_ptr(image), _ptr(out), _ptr(self._workspace(image.device)), width, height, channels, tag, self.scales,
                                 self._threshold_array(channels), self._flags(), _stream())
        check(rc)
        return out

    def process_luminance(self, image: torch.Tensor) -> torch.Tensor:
        """Denoise the Lab lightness of an RGB image and keep a/b (extract -> process -> replace)."""
        lum = extension.compute_luminance(image)
        return extension.modify_luminance(image, self.process(lum.unsqueeze(2)).squeeze(2))

    def process_log_luminance(self, image: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
        """process_luminance on log(max(eps, lightness))."""
        lum = extension.compute_log_luminance(image, eps)
        return extension.modify_log_luminance(image, self.process(lum.unsqueeze(2)).squeeze(2), eps)


__all__ = ['Wavelet']
