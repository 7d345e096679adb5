"""Antialiased image scaling (include/tdk_hip_resample.h: tdk_resample) -- the scaler behind `resize_width`.

Along each axis output i is the average of the source samples under a triangle of half-width r = max(n_in / n_out, 1) centred on
(n_in / n_out) (i + 1/2), normalised by the weights that fall inside the frame: the area-weighted ("antialiased") bilinear
filter when shrinking, plain bilinear interpolation when enlarging, the input's bits at equal size.  Horizontal pass, then
vertical, float32 in between, one rounding at the store.  One kernel launch on PyTorch's current stream, no workspace, no
synchronisation: capturable in a HIP graph from the first call, and bit-reproducible.

    small = Resize(device, (4096, 3072), (1024, 768)).process(frame)      # (H, W, 1 or 3); float32, float16 or uint8
    thumb = Resize.longest_edge(device, (4096, 3072), 256).process(frame)
"""

from __future__ import annotations

import torch

from ._frames import TAGS, check_frame, check_size, require_cuda_device
from ._native import check, lib
from .torch_darktable_extension import _ptr, _stream

MAX_RATIO = 16


class Resize:
    """Scale (H, W, C) images of one size to another; sizes are (width, height).  Shrinking is limited to 16:1 per axis."""

    def __init__(self, device: torch.device, input_size: tuple[int, int], output_size: tuple[int, int]):
        require_cuda_device(device)
        check_size('Input', input_size)
        check_size('Output', output_size)
        (self.width, self.height), (self.out_width, self.out_height) = (int(v) for v in input_size), (int(v) for v in output_size)
        if self.width > MAX_RATIO * self.out_width or self.height > MAX_RATIO * self.out_height:
            raise ValueError(f'ratio {self.width}x{self.height} -> {self.out_width}x{self.out_height} is beyond {MAX_RATIO}:1 on an axis')
        self._device = device

    @staticmethod
    def longest_edge(device: torch.device, input_size: tuple[int, int], longest: int) -> 'Resize':
        """The scaler to `pipeline.util.resize_longest_edge(input_size, longest)` (longest = 0: the same size)."""
        from .pipeline.util import resize_longest_edge  # (the pipeline package imports this module)

        return Resize(device, input_size, resize_longest_edge(input_size, longest))

    @property
    def input_size(self) -> tuple[int, int]:
        return (self.width, self.height)

    @property
    def output_size(self) -> tuple[int, int]:
        return (self.out_width, self.out_height)

    def __repr__(self):
        return f'Resize({self.width}x{self.height} -> {self.out_width}x{self.out_height})'

    def lds_bytes(self, channels: int, dtype: torch.dtype) -> int:
        """LDS one workgroup takes for this geometry (0: not a legal call)."""
        return int(lib.tdk_resample_lds_bytes(self.width, self.height, self.out_width, self.out_height, channels, TAGS.get(dtype, -1)))

    def process(self, image: torch.Tensor) -> torch.Tensor:
        """(height, width, C) -> (out_height, out_width, C), C in {1, 3}, float32, float16 or uint8, the same type out."""
        _, _, channels, tag = check_frame(image, (self.height, self.width), 'Resize')
        with torch.cuda.device(image.device):
            out = torch.empty((self.out_height, self.out_width, channels), dtype=image.dtype, device=image.device)
            rc = lib.tdk_resample(_ptr(image), _ptr(out), self.width, self.height, self.out_width, self.out_height, channels, tag, _stream())
        check(rc)
        return out


__all__ = ['Resize']
