"""Reduced-size demosaic (include/tdk_hip_scaled.h: tdk_demosaic_scaled) -- a raw (H, W) mosaic becomes an (h, w, 3) RGB frame with
h <= H / 2 and w <= W / 2 in one kernel launch that reads the mosaic once; the rest of a chain then runs on a quarter of the pixels
or fewer.

Below half size nothing is demosaiced: every output pixel is the average of the sites of each colour under its footprint, weighted
by `Resize`'s antialiasing triangle laid over all colours on the same centres, so the three channels are registered on one point
(2 x 2 binning leaves red and blue a site apart).  The optional white balance is the one `apply_white_balance` applies, clamp
included; without it samples pass unchanged and values above 1 survive.  One launch on PyTorch's current stream, no workspace, no
synchronisation: capturable in a HIP graph from the first call, and bit-reproducible.

    preview = ScaledDemosaic(device, (4096, 3072), BayerPattern.RGGB, (1024, 768))
    rgb = preview.process(mosaic, white_balance=gains)                       # (768, 1024, 3), the mosaic's float type
    rgb = preview.process_packed(raw_bytes, PackedFormat.Packed12, gains)    # the same from the packed 12-bit bytes
    thumb = ScaledDemosaic.longest_edge(device, (4096, 3072), BayerPattern.RGGB, 512)
"""

from __future__ import annotations

import ctypes

import torch

from ._mosaic import FLOAT_TAGS, MosaicStage, check_gains, check_pattern, out_dtype_of
from ._native import check, lib
from .bayer import BayerPattern, PackedFormat
from .torch_darktable_extension import _pattern, _ptr, _require, _stream

MIN_RATIO, MAX_RATIO = 2, 16
_PACKED = {PackedFormat.Packed12: 0, PackedFormat.Packed12_IDS: 1}


class ScaledDemosaic(MosaicStage):
    """(H, W) mosaics of one size and pattern -> (h, w, 3) frames of one size; sizes are (width, height), the ratio 2..16 per axis."""

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, output_size: tuple[int, int]):
        super().__init__(device, image_size)
        check_pattern(bayer_pattern)
        out_width, out_height = (int(v) for v in output_size)
        if out_width < 1 or out_height < 1:
            raise ValueError(f'Output dimensions must be at least 1x1, got {out_width}x{out_height}')
        if MIN_RATIO * out_width > self.width or MIN_RATIO * out_height > self.height:
            raise ValueError(f'ratio {self.width}x{self.height} -> {out_width}x{out_height} is below {MIN_RATIO}:1 on an axis (a full-size demosaic serves that)')
        if self.width > MAX_RATIO * out_width or self.height > MAX_RATIO * out_height:
            raise ValueError(f'ratio {self.width}x{self.height} -> {out_width}x{out_height} is beyond {MAX_RATIO}:1 on an axis')
        self.bayer_pattern = bayer_pattern
        self.out_width, self.out_height = out_width, out_height

    @staticmethod
    def longest_edge(device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, longest: int) -> 'ScaledDemosaic':
        """The stage to `pipeline.util.resize_longest_edge(image_size, longest)`."""
        from .pipeline.util import resize_longest_edge  # (the pipeline package imports this module)

        return ScaledDemosaic(device, image_size, bayer_pattern, resize_longest_edge(image_size, longest))

    @property
    def output_size(self) -> tuple[int, int]:
        return (self.out_width, self.out_height)

    @property
    def tile(self) -> tuple[int, int]:
        """(columns, rows) of the output tile of one workgroup: it follows from the ratio."""
        tw, th = ctypes.c_int(0), ctypes.c_int(0)
        check(lib.tdk_demosaic_scaled_tile(self.width, self.height, self.out_width, self.out_height, ctypes.byref(tw), ctypes.byref(th)))
        return (tw.value, th.value)

    def __repr__(self):
        return f'ScaledDemosaic({self.width}x{self.height} -> {self.out_width}x{self.out_height}, {self.bayer_pattern.name})'

    def lds_bytes(self) -> int:
        """LDS one workgroup takes (the same for every source and output type)."""
        return int(lib.tdk_demosaic_scaled_lds_bytes(self.width, self.height, self.out_width, self.out_height))

    def process(self, mosaic: torch.Tensor, white_balance: torch.Tensor | None = None, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """(height, width) or (height, width, 1) float32 or float16 mosaic -> (out_height, out_width, 3) of `out_dtype` (None: the
        mosaic's type).  white_balance: None, or a (3,) float32 tensor (R, G, B) on the mosaic's device, read on the device."""
        if mosaic.dim() == 3 and mosaic.shape[-1] == 1:
            mosaic = mosaic[..., 0]
        assert mosaic.dim() == 2, f'mosaic must have 2 dimensions, or 3 with one channel, got {mosaic.shape}'
        self._check_mosaic(mosaic)
        out_dtype = out_dtype_of(out_dtype, mosaic.dtype)
        check_gains(white_balance, mosaic.device)
        with torch.cuda.device(mosaic.device):
            out = torch.empty((self.out_height, self.out_width, 3), dtype=out_dtype, device=mosaic.device)
            rc = lib.tdk_demosaic_scaled(_ptr(mosaic), _ptr(out), _ptr(white_balance), self.width, self.height, self.out_width, self.out_height,
                                         _pattern(self.bayer_pattern), FLOAT_TAGS[mosaic.dtype], FLOAT_TAGS[out_dtype], _stream())
        check(rc)
        return out

    def process_packed(self, payload: torch.Tensor, packed_format: PackedFormat = PackedFormat.Packed12, white_balance: torch.Tensor | None = None,
                       out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """width * height * 3 / 2 packed 12-bit bytes (flat uint8) -> (out_height, out_width, 3): `decode12_float`, the white balance and
        `process` as one launch, with their bits; the width must be even."""
        if packed_format not in _PACKED:
            raise ValueError(f'Unsupported packed format: {packed_format}')
        if self.width % 2:
            raise ValueError(f'the packed form needs an even width (pixel pairs share three bytes), got {self.width}')
        _require(payload.is_cuda, 'Input must be on CUDA device')
        _require(payload.dtype == torch.uint8 and payload.dim() == 1, 'packed input must be a 1-D uint8 tensor')
        _require(payload.is_contiguous(), 'Input must be contiguous')
        expected = self.width * self.height * 3 // 2
        if payload.numel() != expected:
            raise RuntimeError(f'ScaledDemosaic packed input has {payload.numel()} bytes, expected {expected} for {self.width}x{self.height}')
        out_dtype = out_dtype_of(out_dtype, torch.float32)
        check_gains(white_balance, payload.device)
        with torch.cuda.device(payload.device):
            out = torch.empty((self.out_height, self.out_width, 3), dtype=out_dtype, device=payload.device)
            rc = lib.tdk_decode12_demosaic_scaled(_ptr(payload), _ptr(out), _ptr(white_balance), self.width, self.height, self.out_width, self.out_height,
                                                  _pattern(self.bayer_pattern), _PACKED[packed_format], FLOAT_TAGS[out_dtype], _stream())
        check(rc)
        return out


__all__ = ['ScaledDemosaic']
