"""The demosaic for noisy frames (include/tdk_hip_lmmse.h: tdk_lmmse) -- Zhang and Wu's directional linear minimum mean-square-error
demosaic, darktable's LMMSE, which the reference does not have.

Bilinear, PPG and RCD pick a direction per pixel from gradients; on a noisy mosaic they take noise for structure and leave colour
noise that is correlated over several pixels.  Here green minus the other colour is estimated along the row and along the column,

    d      = the directional estimate (a 5-tap interpolation of the missing colour against the sample)
    p      = d low-passed by a 9-tap Gaussian along the same direction
    x, v   = the linear estimate between p and d by their variances over nine sites, and the variance of its error
    D      = (x_h v_v + x_v v_h) / (v_h + v_v)

and red, green and blue follow from D at the site and its neighbours.  By default the arithmetic runs on square roots of the samples,
in which shot noise is about uniform over brightness (`domain='sqrt'`); `domain='linear'` runs it on the samples themselves.  The
exact float32 formulas of the device are in the header, and a NumPy restatement (tests/lmmse_spec.py) predicts the bits.  One kernel,
one launch, no workspace and no synchronisation: capturable in a HIP graph from the first call, and bit-reproducible.

    demosaic = LMMSE(device, (4096, 3072), BayerPattern.RGGB)
    rgb = demosaic.process(mosaic)                           # (H, W) or (H, W, 1) float32 or float16 -> (H, W, 3), the same type
    rgb = demosaic.process(mosaic, out_dtype=torch.float16)  # ... or the type asked for, rounded once
"""

from __future__ import annotations

import torch

from ._frames import require_cuda_device
from ._native import TDK_F16, TDK_F32, TDK_LMMSE_LINEAR, TDK_LMMSE_MAX_SIZE, TDK_LMMSE_MIN_SIZE, TDK_LMMSE_TILE_H, TDK_LMMSE_TILE_W, check, lib
from .bayer import BayerPattern
from .torch_darktable_extension import _pattern, _ptr, _stream

DOMAINS = {'sqrt': 0, 'linear': TDK_LMMSE_LINEAR}
_TAGS = {torch.float32: TDK_F32, torch.float16: TDK_F16}


class LMMSE:
    """LMMSE demosaic for mosaics of one size (width, height) and one Bayer pattern.  domain: 'sqrt' (the default: the estimation
    runs on square roots of the samples, negative samples count as 0) or 'linear'."""

    TILE = (TDK_LMMSE_TILE_W, TDK_LMMSE_TILE_H)  # (width, height) of one workgroup's output tile (csrc/lmmse.hip)

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, *, domain: str = 'sqrt'):
        device = torch.device(device)
        require_cuda_device(device)
        if len(image_size) != 2 or not all(int(v) == v and TDK_LMMSE_MIN_SIZE <= int(v) <= TDK_LMMSE_MAX_SIZE for v in image_size):
            raise ValueError(f'Image dimensions must be integers in {TDK_LMMSE_MIN_SIZE}..{TDK_LMMSE_MAX_SIZE}, got {tuple(image_size)}')
        if not isinstance(bayer_pattern, BayerPattern):
            raise TypeError(f'bayer_pattern must be a BayerPattern, got {type(bayer_pattern).__name__}')
        if domain not in DOMAINS:
            raise ValueError(f"domain must be 'sqrt' or 'linear', got {domain!r}")
        self._device = device
        self.width, self.height = int(image_size[0]), int(image_size[1])
        self._bayer_pattern = bayer_pattern
        self._pattern = _pattern(bayer_pattern)
        self._domain = domain

    @property
    def image_size(self) -> tuple[int, int]:
        return (self.width, self.height)

    @property
    def bayer_pattern(self) -> BayerPattern:
        return self._bayer_pattern

    @property
    def domain(self) -> str:
        return self._domain

    def __repr__(self):
        return f'LMMSE({self.width}x{self.height}, {self._bayer_pattern.name}, domain={self._domain!r})'

    def lds_bytes(self, dtype: torch.dtype = torch.float32, out_dtype: torch.dtype | None = None) -> int:
        """LDS one workgroup takes (0: not a legal call)."""
        return int(lib.tdk_lmmse_lds_bytes(_TAGS.get(dtype, -1), _TAGS.get(dtype if out_dtype is None else out_dtype, -1), DOMAINS[self._domain]))

    def process(self, mosaic: torch.Tensor, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """(H, W) or (H, W, 1) float32 or float16 -> (H, W, 3) in out_dtype (default: the mosaic's type), on the current stream.  The
        site's own colour is the input sample; estimated values are not clamped in the linear domain and >= 0 in the sqrt domain."""
        if not isinstance(mosaic, torch.Tensor):
            raise TypeError(f'mosaic must be a tensor, got {type(mosaic).__name__}')
        if mosaic.dim() not in (2, 3) or (mosaic.dim() == 3 and mosaic.size(2) != 1):
            raise RuntimeError(f'LMMSE input must be (H, W) or (H, W, 1), got {tuple(mosaic.shape)}')
        if tuple(mosaic.shape[:2]) != (self.height, self.width):
            raise RuntimeError(f'LMMSE input shape {tuple(mosaic.shape)} != expected {(self.height, self.width, 1)}')
        if mosaic.dtype not in _TAGS:
            raise RuntimeError(f'Input tensor must be float32 or float16, got {mosaic.dtype}')
        out_dtype = mosaic.dtype if out_dtype is None else out_dtype
        if out_dtype not in _TAGS:
            raise ValueError(f'out_dtype must be float32 or float16, got {out_dtype}')
        if not mosaic.is_cuda:
            raise RuntimeError('Input tensor must be on CUDA device')
        if self._device.index is not None and mosaic.device != self._device:
            raise RuntimeError(f'Input is on {mosaic.device}, the demosaic was built for {self._device}')
        x = mosaic.contiguous()
        with torch.cuda.device(x.device):
            out = torch.empty((self.height, self.width, 3), dtype=out_dtype, device=x.device)
            rc = lib.tdk_lmmse(_ptr(x), _ptr(out), self.width, self.height, self._pattern, _TAGS[x.dtype], _TAGS[out_dtype], DOMAINS[self._domain], _stream())
        check(rc)
        return out


__all__ = ['LMMSE']
