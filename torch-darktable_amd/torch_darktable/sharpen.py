"""Output sharpening (include/tdk_hip_sharpen.h: tdk_sharpen) -- an unsharp mask with darktable's soft threshold and a halo limit.

The signal (each channel, or the luminance of an RGB frame) is blurred by a separable symmetric kernel with the frame's edge
replicated; the detail d = s - blur is shrunk towards zero by `threshold`, scaled by `amount` and added back.  With `overshoot`
the result is held within the 3x3 neighbourhood's minimum and maximum, widened by `overshoot` on both sides, which stops halos at
strong edges.  `threshold` and `overshoot` are in units of the full range: 1.0 is 255 codes of a uint8 frame.  One kernel launch on
PyTorch's current stream, no workspace, no synchronisation: capturable in a HIP graph from the first call, and bit-reproducible.

    crisp = Sharpen(device, sigma=1.0, amount=0.5).process(frame)               # (H, W, 1 or 3); float32, float16 or uint8
    safe = Sharpen(device, sigma=2.0, amount=1.5, threshold=0.01, overshoot=0.02).process(frame)
"""

from __future__ import annotations

import math

import torch

from ._frames import TAGS, check_frame, require_cuda_device
from ._native import TDK_SHARPEN_LIMIT, TDK_SHARPEN_LUMA, TDK_SHARPEN_MAX_RADIUS, check, lib
from ._stage import SeparableTaps
from .torch_darktable_extension import _ptr, _stream

MAX_AMOUNT = 16.0


class Sharpen:
    """Unsharp mask on (H, W, C) images of any size.  `luma` sharpens the luminance of C = 3 frames and adds the same detail to
    all three channels (no colour fringes); it is dropped for C = 1.  `overshoot=None`: no halo limit."""

    TILE = (32, 32)  # (width, height) of one workgroup's output tile (csrc/sharpen.hip: SH_TW, SH_TH)

    def __init__(self, device: torch.device, sigma: float = 1.0, amount: float = 0.5, threshold: float = 0.0, luma: bool = True,
                 overshoot: float | None = None):
        self._setup(device, SeparableTaps.from_sigma(lib.tdk_sharpen_weights, float(sigma), 0.25, 4.0, TDK_SHARPEN_MAX_RADIUS), amount, threshold, luma, overshoot)

    @staticmethod
    def from_weights(device: torch.device, weights, amount: float = 0.5, threshold: float = 0.0, luma: bool = True,
                     overshoot: float | None = None) -> 'Sharpen':
        """A caller's own symmetric kernel: weights (w0, w1, .. wR), 1 <= R <= 12, finite and >= 0, used as float32.  They are
        taken as they are; a blur that keeps a flat area flat needs w0 + 2 (w1 + .. + wR) = 1."""
        self = Sharpen.__new__(Sharpen)
        self._setup(device, weights, amount, threshold, luma, overshoot)
        return self

    def _setup(self, device, weights, amount, threshold, luma, overshoot) -> None:
        require_cuda_device(device)
        self._weights = SeparableTaps.from_values(weights, TDK_SHARPEN_MAX_RADIUS, 'weights')
        self.sigma: float | None = self._weights.sigma
        if not 0.0 <= float(amount) <= MAX_AMOUNT:
            raise ValueError(f'amount must lie in [0, {MAX_AMOUNT:g}], got {amount}')
        if not (math.isfinite(float(threshold)) and float(threshold) >= 0.0):
            raise ValueError(f'threshold must be finite and >= 0, got {threshold}')
        if overshoot is not None and not (math.isfinite(float(overshoot)) and float(overshoot) >= 0.0):
            raise ValueError(f'overshoot must be None or finite and >= 0, got {overshoot}')
        self._device = device
        self.amount, self.threshold, self.luma = float(amount), float(threshold), bool(luma)
        self.overshoot = None if overshoot is None else float(overshoot)

    @property
    def weights(self) -> tuple[float, ...]:
        """The taps w0 .. wR as float32 values."""
        return self._weights.values

    @property
    def radius(self) -> int:
        return self._weights.radius

    def _flags(self, channels: int) -> int:
        return (TDK_SHARPEN_LUMA if self.luma and channels == 3 else 0) | (TDK_SHARPEN_LIMIT if self.overshoot is not None else 0)

    def __repr__(self):
        return f'Sharpen({self._weights!r}, radius={self.radius}, amount={self.amount:g}, threshold={self.threshold:g}, luma={self.luma}, overshoot={self.overshoot})'

    def lds_bytes(self, channels: int, dtype: torch.dtype) -> int:
        """LDS one workgroup takes on frames of this kind (0: not a legal call)."""
        return int(lib.tdk_sharpen_lds_bytes(channels, TAGS.get(dtype, -1), self.radius, self._flags(channels)))

    def process(self, image: torch.Tensor) -> torch.Tensor:
        """(H, W, C) -> (H, W, C), C in {1, 3}, float32, float16 or uint8, the same type out."""
        height, width, channels, tag = check_frame(image)
        with torch.cuda.device(image.device):
            out = torch.empty_like(image)
            rc = lib.tdk_sharpen(_ptr(image), _ptr(out), width, height, channels, tag, self._weights.c_array, self.radius, self.amount,
                                 self.threshold, 0.0 if self.overshoot is None else self.overshoot, self._flags(channels), _stream())
        check(rc)
        return out


__all__ = ['Sharpen']
