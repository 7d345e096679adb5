"""Parametric geometric resampling (include/tdk_hip_warp.h: tdk_warp) -- lens undistortion, rectification, arbitrary rotations
and perspective correction without a coordinate grid.

The map is 18 numbers, `h0..h8, fx, fy, cx, cy, k1, k2, p1, p2, k3`: an output pixel (column u, row v; pixel centres are
integers) goes through the homography h to normalised coordinates, through OpenCV's radial + tangential distortion model and the
camera matrix to a source position, and is interpolated there (bilinear, or bicubic with the Keys kernel A = -0.75 of OpenCV and
torch).  The kernel evaluates the map in registers in float32 in a fixed order; the exact formulas are in the header.  One
launch on PyTorch's current stream, no workspace, no synchronisation: capturable in a HIP graph from the first call, and
bit-reproducible.

    und = Warp.undistort(device, (4096, 3072), K, dist)                      # cv2.initUndistortRectifyMap + cv2.remap
    out = und.process(frame)                                                 # (H, W, 1 or 3); float32, float16 or uint8
    rot = Warp.homography(device, (w, h), (w, h), H, border='replicate')     # H: output pixel -> source pixel
    pts = und.coordinates()                                                  # (H, W, 2): where every output pixel samples

The warp point-samples its interpolation kernel: it does not low-pass a source that it shrinks.  For antialiased minification
use `Resize` (before or after the warp).
"""

from __future__ import annotations

import ctypes
import math
from typing import Sequence

import numpy as np
import torch

from ._frames import TAGS, check_frame, check_size, require_cuda_device
from ._native import TDK_WARP_DIRECT, check, lib
from .torch_darktable_extension import _ptr, _stream

_INTERPOLATION = {'bilinear': 0, 'bicubic': 1}
_BORDER = {'constant': 0, 'replicate': 1}


def _matrix3(value, what: str) -> np.ndarray:
    m = np.asarray(value, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError(f'{what} must be 3x3, got shape {m.shape}')
    return m


class Warp:
    """Resample (H, W, C) images of one size through an 18-number map to another size; sizes are (width, height)."""

    def __init__(self, device: torch.device, input_size: tuple[int, int], output_size: tuple[int, int], map: Sequence[float],
                 interpolation: str = 'bicubic', border: str = 'constant', fill: float = 0.0):
        require_cuda_device(device)
        check_size('Input', input_size)
        check_size('Output', output_size)
        (self.width, self.height), (self.out_width, self.out_height) = (int(v) for v in input_size), (int(v) for v in output_size)
        if interpolation not in _INTERPOLATION:
            raise ValueError(f"interpolation must be 'bilinear' or 'bicubic', got {interpolation!r}")
        if border not in _BORDER:
            raise ValueError(f"border must be 'constant' or 'replicate', got {border!r}")
        values = np.asarray(map, dtype=np.float64).reshape(-1)
        if values.size != 18:
            raise ValueError(f'map must have 18 entries (h0..h8, fx, fy, cx, cy, k1, k2, p1, p2, k3), got {values.size}')
        with np.errstate(over='ignore'):
            self._map = values.astype(np.float32)   # the one rounding of whatever the host computed in float64
        if not np.isfinite(self._map).all():
            raise ValueError('map entries must be finite in float32')
        if not math.isfinite(float(fill)):
            raise ValueError(f'fill must be finite, got {fill}')
        self.interpolation, self.border, self.fill = interpolation, border, float(fill)
        self._c_map = (ctypes.c_float * 18)(*self._map.tolist())
        self._device = device

    @staticmethod
    def undistort(device: torch.device, size: tuple[int, int], camera_matrix, dist_coeffs, new_camera_matrix=None, rectify=None,
                  output_size: tuple[int, int] | None = None, **kw) -> 'Warp':
        """The map of OpenCV's initUndistortRectifyMap: the output is the view of an ideal camera `new_camera_matrix` (default:
        camera_matrix) rotated by `rectify` (R, default: none); h = inv(new_camera_matrix @ R) in float64, rounded once.
        dist_coeffs: (k1, k2, p1, p2[, k3])."""
        K = _matrix3(camera_matrix, 'camera_matrix')
        Knew = K if new_camera_matrix is None else _matrix3(new_camera_matrix, 'new_camera_matrix')
        R = np.eye(3) if rectify is None else _matrix3(rectify, 'rectify')
        d = np.asarray(dist_coeffs, dtype=np.float64).reshape(-1)
        if d.size not in (4, 5):
            raise ValueError(f'dist_coeffs must have 4 or 5 entries (k1, k2, p1, p2[, k3]), got {d.size}: the rational and fisheye models are not supported')
        k1, k2, p1, p2 = d[:4]
        k3 = d[4] if d.size == 5 else 0.0
        h = np.linalg.inv(Knew @ R)
        values = [*h.reshape(-1), K[0, 0], K[1, 1], K[0, 2], K[1, 2], k1, k2, p1, p2, k3]
        return Warp(device, size, size if output_size is None else output_size, values, **kw)

    @staticmethod
    def homography(device: torch.device, input_size: tuple[int, int], output_size: tuple[int, int], H, **kw) -> 'Warp':
        """H maps an output pixel (u, v, 1) to a source pixel (X / Z, Y / Z); the identity returns the input."""
        h = _matrix3(H, 'H')
        return Warp(device, input_size, output_size, [*h.reshape(-1), 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], **kw)

    @staticmethod
    def from_transform(device: torch.device, size: tuple[int, int], transform, **kw) -> 'Warp':
        """The orientation `pipeline.transform.transform(image, transform)` applies, as a homography with integer entries."""
        from .pipeline.transform import ImageTransform, transformed_size  # (the pipeline package imports this package)

        w, h = (int(v) for v in size)
        T = ImageTransform
        H = {
            T.none: [[1, 0, 0], [0, 1, 0]],
            T.rotate_90: [[0, -1, w - 1], [1, 0, 0]],
            T.rotate_180: [[-1, 0, w - 1], [0, -1, h - 1]],
            T.rotate_270: [[0, 1, 0], [-1, 0, h - 1]],
            T.transpose: [[0, 1, 0], [1, 0, 0]],
            T.flip_horiz: [[-1, 0, w - 1], [0, 1, 0]],
            T.flip_vert: [[1, 0, 0], [0, -1, h - 1]],
            T.transverse: [[-1, 0, w - 1], [0, -1, h - 1]],
        }[T(transform)]
        return Warp.homography(device, (w, h), transformed_size((w, h), T(transform)), [*H, [0, 0, 1]], **kw)

    @property
    def input_size(self) -> tuple[int, int]:
        return (self.width, self.height)

    @property
    def output_size(self) -> tuple[int, int]:
        return (self.out_width, self.out_height)

    @property
    def map(self) -> np.ndarray:
        """The 18 float32 values the kernel gets (a copy)."""
        return self._map.copy()

    def __repr__(self):
        return (f'Warp({self.width}x{self.height} -> {self.out_width}x{self.out_height}, {self.interpolation}, {self.border}'
                + (f', fill={self.fill:g}' if self.border == 'constant' or self.fill else '') + ')')

    def lds_bytes(self, channels: int, dtype: torch.dtype) -> int:
        """LDS one workgroup takes (0: not a legal call)."""
        return int(lib.tdk_warp_lds_bytes(channels, TAGS.get(dtype, -1), _INTERPOLATION[self.interpolation]))

    def process(self, image: torch.Tensor, direct: bool = False) -> torch.Tensor:
        """(height, width, C) -> (out_height, out_width, C), C in {1, 3}, float32, float16 or uint8, the same type out.
        direct=True (TDK_WARP_DIRECT) makes every tile sample from global memory: the same bits, for tests and measurement."""
        _, _, channels, tag = check_frame(image, (self.height, self.width), 'Warp')
        with torch.cuda.device(image.device):
            out = torch.empty((self.out_height, self.out_width, channels), dtype=image.dtype, device=image.device)
            rc = lib.tdk_warp(_ptr(image), _ptr(out), self.width, self.height, self.out_width, self.out_height, channels, tag,
                              ctypes.addressof(self._c_map), _INTERPOLATION[self.interpolation], _BORDER[self.border], self.fill,
                              TDK_WARP_DIRECT if direct else 0, _stream())
        check(rc)
        return out

    def coordinates(self) -> torch.Tensor:
        """(out_height, out_width, 2) float32: the source position (sx, sy) of every output pixel before it is clamped to the
        frame, NaN in both where the pixel is outside (Z <= 0 or a non-finite position).  For remapping keypoints and masks."""
        with torch.cuda.device(self._device):
            xy = torch.empty((self.out_height, self.out_width, 2), dtype=torch.float32, device=self._device)
            rc = lib.tdk_warp_coordinates(_ptr(xy), self.out_width, self.out_height, ctypes.addressof(self._c_map), _stream())
        check(rc)
        return xy


__all__ = ['Warp']
