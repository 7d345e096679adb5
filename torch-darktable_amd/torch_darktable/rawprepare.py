"""Sensor correction at the head of the chain (include/tdk_hip_raw.h: tdk_raw_prepare) -- black and white level, defective
pixels, lens shading, white balance and clip, from packed or unpacked mosaic to the corrected (H, W) mosaic in one kernel.

    L = (raw - black[p]) * scale[p]            p = 2*(row & 1) + (column & 1), scale[p] = 1 / (white - black[p])
    hot / dead sites are replaced from their four same-colour neighbours two sites away (decided on the uncorrected frame)
    the value is multiplied by a bilinear gain grid per CFA position (DNG GainMap semantics: the grid spans the frame)
    white balance and the clamp to [0, 1], in the operation order of apply_white_balance

The exact float32 formulas are in the header; a NumPy restatement (tests/test_rawprepare_spec.py) predicts the bits.  One launch
on PyTorch's current stream, no workspace, no synchronisation: capturable in a HIP graph from the first call, bit-reproducible.

    rp = RawPrepare(device, (4096, 3072), BayerPattern.RGGB, black=256.0, white=4095.0, hot=True, dead=True,
                    shading=RawPrepare.shading_from_rgb(flat_field_gains, BayerPattern.RGGB))
    mosaic = rp.process_packed(raw_bytes, PackedFormat.Packed12, white_balance=gains)      # (H, W) float32
    rgb = RCD(device, (4096, 3072), BayerPattern.RGGB).process(mosaic.unsqueeze(-1))

`threshold` is in the units of L (1.0 = white level).  With black = 0, white = 4095 and nothing else enabled `process_packed`
returns the bits of `decode12_float`; with `white_balance` added, those of `apply_white_balance` on it.
"""

from __future__ import annotations

import ctypes
import math
from typing import Sequence

import numpy as np
import torch

from ._mosaic import FLOAT_TAGS, MosaicStage, check_pattern, out_dtype_of
from ._native import (TDK_RAW_DEAD, TDK_RAW_F16, TDK_RAW_F32, TDK_RAW_HOT, TDK_RAW_PACKED12, TDK_RAW_PACKED12_IDS, TDK_RAW_U16, check, lib)
from .bayer import BayerPattern, PackedFormat
from .torch_darktable_extension import _pattern, _ptr, _require, _stream

MAX_GRID = 257
_IN_FORMATS = {torch.uint16: TDK_RAW_U16, torch.float32: TDK_RAW_F32, torch.float16: TDK_RAW_F16}
_PACKED = {PackedFormat.Packed12: TDK_RAW_PACKED12, PackedFormat.Packed12_IDS: TDK_RAW_PACKED12_IDS}


def _positions(pattern: BayerPattern) -> tuple[int, int, int, int]:
    """Colour (0 = R, 1 = G, 2 = B) of the four CFA positions p = 2*(row & 1) + (column & 1)."""
    word = _pattern(pattern)
    return tuple((word >> (2 * p)) & 3 for p in range(4))


class RawPrepare(MosaicStage):
    """Correct (H, W) mosaics of one size; image_size is (width, height), both even."""

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, black: float | Sequence[float] = 0.0,
                 white: float = 4095.0, shading: torch.Tensor | None = None, hot: bool = False, dead: bool = False, threshold: float = 0.02,
                 ratio: float = 0.5, min_count: int = 3, clip: bool = True):
        super().__init__(device, image_size)
        self._check_even('Image')
        check_pattern(bayer_pattern)
        levels = np.asarray(black, dtype=np.float64).reshape(-1)
        if levels.size == 1:
            levels = np.repeat(levels, 4)
        if levels.size != 4:
            raise ValueError(f'black must be one level or four (one per CFA position), got {levels.size}')
        if not (np.isfinite(levels).all() and math.isfinite(float(white))):
            raise ValueError('black and white must be finite')
        if not (float(white) > levels).all():
            raise ValueError(f'white ({white}) must lie above every black level ({levels.tolist()})')
        with np.errstate(over='ignore'):
            self._black = levels.astype(np.float32)
            self._scale = (1.0 / (float(white) - levels)).astype(np.float32)   # float64 on the host, rounded once
        if not (np.isfinite(self._black).all() and np.isfinite(self._scale).all()):
            raise ValueError('black and 1 / (white - black) must be finite in float32')
        if not (math.isfinite(float(threshold)) and float(threshold) >= 0.0):
            raise ValueError(f'threshold must be finite and >= 0, got {threshold}')
        if not 0.0 < float(ratio) <= 1.0:
            raise ValueError(f'ratio must lie in (0, 1], got {ratio}')
        if int(min_count) != min_count or not 1 <= int(min_count) <= 4:
            raise ValueError(f'min_count must be 1..4, got {min_count}')
        self.bayer_pattern = bayer_pattern
        self.white = float(white)
        self.hot, self.dead, self.clip = bool(hot), bool(dead), bool(clip)
        self.threshold, self.ratio, self.min_count = float(threshold), float(ratio), int(min_count)
        self._shading: torch.Tensor | None = None
        if shading is not None:
            if shading.dim() != 3 or shading.size(2) != 4:
                raise ValueError(f'shading must be (grid_height, grid_width, 4), got {tuple(shading.shape)}')
            gh, gw = shading.size(0), shading.size(1)
            if not (2 <= gw <= MAX_GRID and 2 <= gh <= MAX_GRID):
                raise ValueError(f'shading grid must be 2..{MAX_GRID} nodes per axis, got {gw}x{gh}')
            if 4 * (gw - 1) > self.width - 1 or 4 * (gh - 1) > self.height - 1:
                raise ValueError(f'shading grid {gw}x{gh} too dense for a {self.width}x{self.height} frame (nodes must be at least 4 pixels apart)')
            self._shading = shading.to(device=device, dtype=torch.float32).contiguous()
        self._c_black = (ctypes.c_float * 4)(*self._black.tolist())
        self._c_scale = (ctypes.c_float * 4)(*self._scale.tolist())

    @staticmethod
    def shading_from_rgb(gains_hw3: torch.Tensor, bayer_pattern: BayerPattern) -> torch.Tensor:
        """(gh, gw, 3) gains per colour (R, G, B) -> (gh, gw, 4) gains per CFA position of `bayer_pattern`."""
        if gains_hw3.dim() != 3 or gains_hw3.size(2) != 3:
            raise ValueError(f'gains must be (grid_height, grid_width, 3), got {tuple(gains_hw3.shape)}')
        return gains_hw3[:, :, list(_positions(bayer_pattern))].to(torch.float32).contiguous()

    @property
    def black(self) -> np.ndarray:
        """The four float32 black levels the kernel gets (a copy)."""
        return self._black.copy()

    @property
    def scale(self) -> np.ndarray:
        """The four float32 factors 1 / (white - black[p]) the kernel gets (a copy)."""
        return self._scale.copy()

    @property
    def shading(self) -> torch.Tensor | None:
        return self._shading

    def __repr__(self):
        steps = [f'black={self._black.tolist()}', f'white={self.white:g}']
        if self.hot or self.dead:
            steps.append(f'defects={"+".join(n for n, on in (("hot", self.hot), ("dead", self.dead)) if on)}'
                         f'(threshold={self.threshold:g}, ratio={self.ratio:g}, min_count={self.min_count})')
        if self._shading is not None:
            steps.append(f'shading={self._shading.size(1)}x{self._shading.size(0)}')
        return f'RawPrepare({self.width}x{self.height}, {self.bayer_pattern.name}, {", ".join(steps)}, clip={self.clip})'

    def lds_bytes(self, mask: bool = False) -> int:
        """LDS one workgroup takes (0: the plain streaming form)."""
        return int(lib.tdk_raw_prepare_lds_bytes(int(self.hot or self.dead or mask), int(self._shading is not None)))

    def _run(self, src: torch.Tensor, src_format: int, white_balance, out_dtype: torch.dtype, mask_out: torch.Tensor | None) -> torch.Tensor:
        out_dtype_of(out_dtype, None)
        gains = None
        if white_balance is not None:
            gains = torch.as_tensor(white_balance).to(device=src.device, dtype=torch.float32).contiguous()
            if gains.numel() != 3:
                raise ValueError(f'white_balance must have 3 elements (R, G, B), got {gains.numel()}')
        if mask_out is not None:
            if tuple(mask_out.shape) != (self.height, self.width):
                raise RuntimeError(f'RawPrepare mask shape {tuple(mask_out.shape)} != expected {(self.height, self.width)}')
            _require(mask_out.is_cuda and mask_out.device == src.device, 'mask_out must be on the input\'s CUDA device')
            _require(mask_out.dtype == torch.uint8 and mask_out.is_contiguous(), 'mask_out must be a contiguous uint8 tensor')
        shading = self._shading
        if shading is not None and shading.device != src.device:
            raise RuntimeError(f'RawPrepare was built for {shading.device}, the input is on {src.device}')
        with torch.cuda.device(src.device):
            out = torch.empty((self.height, self.width), dtype=out_dtype, device=src.device)
            rc = lib.tdk_raw_prepare(_ptr(src), src_format, _ptr(out), FLOAT_TAGS[out_dtype], _ptr(mask_out), self.width, self.height,
                                     _pattern(self.bayer_pattern), ctypes.addressof(self._c_black), ctypes.addressof(self._c_scale),
                                     (TDK_RAW_HOT if self.hot else 0) | (TDK_RAW_DEAD if self.dead else 0), self.threshold, self.ratio, self.min_count,
                                     _ptr(shading), shading.size(1) if shading is not None else 0, shading.size(0) if shading is not None else 0,
                                     _ptr(gains), int(self.clip), _stream())
        check(rc)
        return out

    def process(self, mosaic: torch.Tensor, white_balance=None, out_dtype: torch.dtype = torch.float32, mask_out: torch.Tensor | None = None) -> torch.Tensor:
        """(height, width) uint16 codes, float32 or float16 -> corrected (height, width) mosaic of `out_dtype`.  black and white are in
        the input's units, `threshold` in those of L.  white_balance: 3 gains (R, G, B); a float32 tensor on the device keeps the
        call free of copies.  mask_out: (height, width) uint8, receives 0 / 1 (hot) / 2 (dead)."""
        assert mosaic.dim() == 2, f'mosaic must have 2 dimensions, got {mosaic.shape}'
        self._check_mosaic(mosaic, 'input', _IN_FORMATS, 'uint16, float32 or float16')
        return self._run(mosaic, _IN_FORMATS[mosaic.dtype], white_balance, out_dtype, mask_out)

    def process_packed(self, bytes: torch.Tensor, format_type: PackedFormat = PackedFormat.Packed12, white_balance=None,
                       out_dtype: torch.dtype = torch.float32, mask_out: torch.Tensor | None = None) -> torch.Tensor:
        """width * height * 3 / 2 packed bytes (flat uint8) -> corrected (height, width) mosaic; black and white in 12-bit codes."""
        if format_type not in _PACKED:
            raise ValueError(f'Unsupported packed format: {format_type}')
        _require(bytes.is_cuda, 'Input must be on CUDA device')
        _require(bytes.dtype == torch.uint8 and bytes.dim() == 1, 'packed input must be a 1-D uint8 tensor')
        _require(bytes.is_contiguous(), 'Input must be contiguous')
        expected = self.width * self.height * 3 // 2
        if bytes.numel() != expected:
            raise RuntimeError(f'RawPrepare packed input has {bytes.numel()} bytes, expected {expected} for {self.width}x{self.height}')
        return self._run(bytes, _PACKED[format_type], white_balance, out_dtype, mask_out)


__all__ = ['RawPrepare']
