"""Argument checks shared by the operators on (H, W, C) frames of float32, float16 or uint8 with 1 or 3 channels: Resize, Warp, Sharpen."""

from __future__ import annotations

import torch

from ._native import TDK_F16, TDK_F32, TDK_U8
from .torch_darktable_extension import _require

MAX_SIZE = 65535
TAGS = {torch.float32: TDK_F32, torch.float16: TDK_F16, torch.uint8: TDK_U8}


def require_cuda_device(device: torch.device) -> None:
    if device.type != 'cuda':
        raise ValueError(f'Device must be CUDA, got {device}')


def check_size(what: str, size) -> None:
    """size is (width, height)."""
    if not all(1 <= int(v) <= MAX_SIZE for v in size):
        raise ValueError(f'{what} dimensions must be 1..{MAX_SIZE}, got {size[0]}x{size[1]}')


def check_frame(image: torch.Tensor, expected_hw: tuple[int, int] | None = None, what: str = '') -> tuple[int, int, int, int]:
    """(height, width, channels, dtype tag) of a frame the kernels take.  expected_hw: the (height, width) an operator `what` was built
    for; None: any size a kernel takes."""
    assert image.dim() == 3, f'image must have 3 dimensions, got {image.shape}'
    height, width, channels = image.shape
    if expected_hw is not None and (height, width) != tuple(expected_hw):
        raise RuntimeError(f'{what} input shape {tuple(image.shape)} != expected {(*expected_hw, channels)}')
    if channels not in {1, 3}:
        raise ValueError(f'image channels must be 1 or 3, got {channels}')
    if expected_hw is None:
        check_size('image', (width, height))
    _require(image.is_cuda, 'Input must be on CUDA device')
    _require(image.is_contiguous(), 'Input must be contiguous')
    _require(image.dtype in TAGS, 'Input tensor must be float32, float16 or uint8')
    return height, width, channels, TAGS[image.dtype]
