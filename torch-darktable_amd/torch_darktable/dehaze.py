"""Haze removal (include/tdk_hip_dehaze.h: tdk_dehaze, tdk_dehaze_ambient) -- He et al.'s dark channel prior with a guided transmission
map, the stage darktable calls haze removal.

Haze, dust and spray add a veil A*(1 - t) to the scene and attenuate it by the transmission t, which falls with distance.  No tone
curve removes that: the correction differs per depth and must stop at depth edges.

    m_c, M_c, L = minimum and mean of max(x_c, 0), mean of the luminance Y, over cells of `cell` x `cell` pixels
    A           = mean of M over the cells whose dark channel (windowed minimum of min_c m_c) is among the K largest, ties included
    t           = 1 - strength * min(windowed minimum of min_c m_c / A_c, 1)
    a, b        = filter of t guided by L (He et al.): box windows of (2*radius + 1)^2 cells, a = cov(L, t) / (var(L) + eps)
    tp          = clamp(up(box(a)) * Y + up(box(b)), floor, 1)              bilinear between cell centres
    out         = max((x - A) / tp + A, 0)

The exact float32 formulas of the device are in the header, and a NumPy restatement (tests/dehaze_spec.py) predicts the bits, those of
the ambient light included: the K largest are found by a radix select that takes every tie, and the means are integer sums.  Five
launches on PyTorch's current stream with the estimate, three with an ambient light that is given; no synchronisation.  The ambient
light is read from device memory by every call, so a captured call follows a tensor that is rewritten.  The workspace belongs to the
object, one per stream: capturable in a HIP graph from the first call, and bit-reproducible.

    dh = Dehaze(device, (4096, 3072))
    out = dh.process(rgb)                          # (H, W, 3) float32 or float16, the same type out; not clamped above
    A = dh.estimate_ambient(rgb)                   # (4,) float32 on the device: A_r, A_g, A_b, the cells averaged
    out = dh.process(other, ambient=A)             # the ambient light of one frame for the next ones
"""

from __future__ import annotations

import math

import torch

from ._frames import TAGS
from ._native import TDK_DEHAZE_MAX_CELLS, TDK_DEHAZE_MAX_DARK_RADIUS, TDK_DEHAZE_MAX_RADIUS, check, lib
from ._stage import FrameStage, as_float32, luma_weights
from .torch_darktable_extension import _ptr, _stream

CELLS = (2, 4, 8, 16)
MIN_FLOOR = 2.0 ** -6


class Dehaze(FrameStage):
    """Remove haze from (H, W, 3) frames of one size (width, height).  strength: how much of the estimated haze goes (1: all of it,
    which looks flat; 0: none); floor: the least transmission divided by; dark_radius, radius: the windows of the dark channel and of
    the guided filter, in cells; quantile: the share of cells, the haziest, whose mean is the ambient light."""

    TILE = (128, 32)  # (width, height) of one workgroup's tile in the apply launch (csrc/dehaze.hip: DH_TW, DH_TH)

    def __init__(self, device: torch.device, image_size: tuple[int, int], strength: float = 0.9, floor: float = 0.1, cell: int = 8, dark_radius: int = 1,
                 radius: int = 4, eps: float = 1e-3, quantile: float = 0.01, weights=None):
        super().__init__(device, image_size)
        if cell not in CELLS:
            raise ValueError(f'cell must be one of {CELLS}, got {cell}')
        cells = -(-self.width // cell) * -(-self.height // cell)
        if cells > TDK_DEHAZE_MAX_CELLS:
            raise ValueError(f'the grid of {cells} cells is larger than {TDK_DEHAZE_MAX_CELLS}: use a larger cell')
        if int(dark_radius) != dark_radius or not 0 <= int(dark_radius) <= TDK_DEHAZE_MAX_DARK_RADIUS:
            raise ValueError(f'dark_radius must be an integer in 0..{TDK_DEHAZE_MAX_DARK_RADIUS}, got {dark_radius}')
        if int(radius) != radius or not 0 <= int(radius) <= TDK_DEHAZE_MAX_RADIUS:
            raise ValueError(f'radius must be an integer in 0..{TDK_DEHAZE_MAX_RADIUS}, got {radius}')
        eps = as_float32(eps)
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError(f'eps must be finite and > 0 as a float32, got {eps}')
        strength = as_float32(strength)
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f'strength must be in 0..1, got {strength}')
        floor = as_float32(floor)
        if not MIN_FLOOR <= floor <= 1.0:
            raise ValueError(f'floor must be in 2^-6..1, got {floor}')
        quantile = float(quantile)
        if not 0.0 < quantile <= 1.0:
            raise ValueError(f'quantile must be in (0, 1], got {quantile}')
        self.weights, self._c_weights = luma_weights(weights)
        self.cell, self.dark_radius, self.radius = int(cell), int(dark_radius), int(radius)
        self.eps, self.strength, self.floor, self.quantile = eps, strength, floor, quantile
        self.cells = cells
        self.count = max(1, math.floor(quantile * cells))   # K: the cells whose mean is the ambient light, before ties
        self._fixed = False                       # True: set_ambient gave the ambient light, calls do not estimate
        self._host_ambient = torch.zeros(4, dtype=torch.float32)   # kept by the object: set_ambient copies from it in stream order
        where = self._prepare()
        self._ambient: torch.Tensor | None = None if where is None else torch.zeros(4, dtype=torch.float32, device=where)

    @property
    def ambient(self) -> torch.Tensor | None:
        """The object's (4,) float32 device tensor A_r, A_g, A_b, cells averaged: what the last estimating call left, or what
        set_ambient put there (None where no GPU exists)."""
        return self._ambient

    @property
    def ambient_is_fixed(self) -> bool:
        return self._fixed

    def __repr__(self):
        return (f'Dehaze({self.width}x{self.height}, strength={self.strength:g}, floor={self.floor:g}, cell={self.cell}, dark_radius={self.dark_radius}, '
                f'radius={self.radius}, eps={self.eps:g}, quantile={self.quantile:g})')

    def workspace_bytes(self) -> int:
        return int(lib.tdk_dehaze_workspace_bytes(self.width, self.height, self.cell))

    def lds_bytes(self, dtype: torch.dtype = torch.float32) -> int:
        """The largest LDS use of a workgroup over the launches of a call on frames of this type (0: not a legal call)."""
        return int(lib.tdk_dehaze_lds_bytes(TAGS.get(dtype, -1), self.cell, self.dark_radius, self.radius))

    def set_ambient(self, ambient) -> None:
        """A fixed ambient light for the calls that follow: three values, or a tensor of three or four (a device tensor is copied on
        the device), copied in stream order into the object's tensor, so replays of a captured call see it.  None: estimate per call
        again."""
        if ambient is None:
            self._fixed = False
            return
        if isinstance(ambient, torch.Tensor):
            if ambient.dtype != torch.float32 or ambient.dim() != 1 or ambient.numel() not in (3, 4):
                raise ValueError(f'ambient must be a float32 tensor of 3 or 4 values, got {ambient.dtype} {tuple(ambient.shape)}')
            source = ambient
        else:
            values = tuple(float(v) for v in ambient)
            if len(values) != 3 or not all(math.isfinite(v) for v in values):
                raise ValueError(f'ambient must be three finite values, a tensor or None, got {ambient}')
            self._host_ambient.copy_(torch.tensor((*values, 0.0), dtype=torch.float32))
            source = self._host_ambient
        if self._ambient is not None:
            self._ambient[:source.numel()].copy_(source, non_blocking=True)
        self._fixed = True

    def _check(self, image: torch.Tensor, ambient):
        height, width, _, tag = self._float_frame(image, 'Dehaze', 'image channels must be 3')
        if self._ambient is None or self._ambient.device != image.device:
            raise RuntimeError(f'Dehaze was built for {None if self._ambient is None else self._ambient.device}, the image is on {image.device}')
        if ambient is not None:
            if not isinstance(ambient, torch.Tensor) or ambient.dtype != torch.float32 or tuple(ambient.shape) != (4,) or not ambient.is_contiguous():
                raise ValueError('ambient must be a contiguous (4,) float32 tensor (what estimate_ambient returns) or None')
            if ambient.device != image.device:
                raise RuntimeError(f'ambient is on {ambient.device}, the image on {image.device}')
        return height, width, tag

    def _run(self, image: torch.Tensor, ambient, want_frame: bool, want_transmission: bool):
        height, width, tag = self._check(image, ambient)
        count = 0 if (ambient is not None or self._fixed) else self.count
        with torch.cuda.device(image.device):
            out = torch.empty_like(image) if want_frame else None
            t = torch.empty((height, width), dtype=torch.float32, device=image.device) if want_transmission else None
            rc = lib.tdk_dehaze(_ptr(image), _ptr(out), _ptr(t), _ptr(self._workspace(image.device)), _ptr(self._ambient if ambient is None else ambient), width,
                                height, tag, self.cell, self.dark_radius, self.radius, count, self.eps, self.strength, self.floor, self._c_weights, 0, _stream())
        check(rc)
        return out, t

    def process(self, image: torch.Tensor, ambient: torch.Tensor | None = None, return_transmission: bool = False):
        """(H, W, 3) float32 or float16 -> the frame of the same type without its haze, not clamped above.  ambient: a (4,) float32
        device tensor that is read on the device (three launches); None: the fixed ambient light if set_ambient gave one, else it is
        estimated from this frame and left in `ambient` (five launches).  return_transmission: (frame, t) with the (H, W) float32
        clamped transmission divided by."""
        out, t = self._run(image, ambient, True, bool(return_transmission))
        return (out, t) if return_transmission else out

    def transmission(self, image: torch.Tensor, ambient: torch.Tensor | None = None) -> torch.Tensor:
        """The (H, W) float32 clamped transmission alone: no frame is written."""
        return self._run(image, ambient, False, True)[1]

    def estimate_ambient(self, image: torch.Tensor) -> torch.Tensor:
        """A new (4,) float32 device tensor A_r, A_g, A_b, cells averaged, of this frame (three launches).  The object's own
        tensor and a fixed ambient light stay as they are."""
        height, width, tag = self._check(image, None)
        with torch.cuda.device(image.device):
            ambient = torch.empty(4, dtype=torch.float32, device=image.device)
            rc = lib.tdk_dehaze_ambient(_ptr(image), _ptr(ambient), _ptr(self._workspace(image.device)), width, height, tag, self.cell, self.dark_radius, self.count, 0,
                                        _stream())
        check(rc)
        return ambient


__all__ = ['Dehaze']
