"""Purple-fringe removal (include/tdk_hip_defringe.h: tdk_defringe) -- the rule of darktable's defringe module on demosaiced frames,
with a frame-wide threshold.

Red and blue are focused a little off green; next to a clipped highlight they spill over dark structure as a purple or blue halo a
few pixels wide, which no radial model removes (ChromaticAberration shifts channels, it does not refocus them).  In the space
(Y, Cb, Cr) = (r/4 + g/2 + b/4, b - g, r - g) of the square roots of the samples:

    E      = |C - G(C)|^2                                   G: the separable blur with the taps, the frame's edge replicated
    th     = max(floor, strength * mean(min(E, 1024)))      mode 'static': max(floor, strength)
    C'     = sum(C_s / (E_s + th)) / sum(1 / (E_s + th))    over the disc of `radius` around a pixel with E > th
    out    = (Y, C') back in RGB where E > th, the input's bits elsewhere

The exact float32 formulas of the device are in the header, and a NumPy restatement (tests/defringe_spec.py) predicts the bits.  Two
kernels: one writes E and a partial sum of the statistic per workgroup, the other forms th and rewrites the fringed pixels.  No
synchronisation: capturable in a HIP graph from the first call, and bit-reproducible.

    d = Defringe(device, (4096, 3072))
    clean = d.process(rgb)                           # (H, W, 3) float32 or float16, the same type out
    clean, m = d.process(rgb, return_mask=True)      # m: (H, W) uint8, 1 where a pixel was rewritten
    s, th = d.threshold()                            # device tensors: the statistic and the threshold of the last call on this stream
"""

from __future__ import annotations

import math

import torch

from ._frames import TAGS
from ._native import (TDK_DEFRINGE_GROUPS_SHIFT, TDK_DEFRINGE_LINEAR, TDK_DEFRINGE_MAX_GROUPS, TDK_DEFRINGE_MAX_RADIUS, TDK_DEFRINGE_MAX_SAMPLE_RADIUS,
                      TDK_DEFRINGE_STATIC, TDK_DEFRINGE_TILE, check, lib)
from ._stage import FrameStage, SeparableTaps, as_float32
from .torch_darktable_extension import _ptr, _stream

MODES = ('global', 'static')
DOMAINS = ('sqrt', 'linear')
STATS_BYTES = 16   # tdk_defringe_stats: S as 64 bits, th as float32, a reserved word


class Defringe(FrameStage):
    """Defringe (H, W, 3) frames of one size (width, height).  sigma: the Gaussian that defines "the chroma around a pixel"; radius:
    S_r, the disc a fringed pixel's new chroma is averaged over; strength: the threshold in units of the frame's average edge chroma
    (mode 'global') or the threshold itself (mode 'static'); floor: the least threshold; domain: the values the stage works on,
    square roots of the samples or the samples."""

    TILE = (TDK_DEFRINGE_TILE, TDK_DEFRINGE_TILE)  # (width, height) of one workgroup's output tile (csrc/defringe.hip: DF_T)
    _record_bytes = STATS_BYTES

    def __init__(self, device: torch.device, image_size: tuple[int, int], sigma: float = 2.0, radius: int = 6, strength: float = 2.5, floor: float = 1e-4,
                 mode: str = 'global', domain: str = 'sqrt'):
        taps = SeparableTaps.from_sigma(lib.tdk_defringe_weights, as_float32(sigma), 0.5, 4.0, TDK_DEFRINGE_MAX_RADIUS)
        self._setup(device, image_size, taps, radius, strength, floor, mode, domain)

    @staticmethod
    def from_weights(device: torch.device, image_size: tuple[int, int], taps, radius: int = 6, strength: float = 2.5, floor: float = 1e-4, mode: str = 'global',
                     domain: str = 'sqrt') -> 'Defringe':
        """A caller's own symmetric blur: taps (w0, w1, .. wR), 1 <= R <= 12, finite and >= 0, used as float32.  They are taken as
        they are; a blur that keeps a flat area flat needs w0 + 2 (w1 + .. + wR) = 1."""
        self = Defringe.__new__(Defringe)
        self._setup(device, image_size, taps, radius, strength, floor, mode, domain)
        return self

    def _setup(self, device, image_size, taps, radius, strength, floor, mode, domain) -> None:
        super().__init__(device, image_size)
        self._taps = SeparableTaps.from_values(taps, TDK_DEFRINGE_MAX_RADIUS, 'taps')
        self.sigma: float | None = self._taps.sigma
        if int(radius) != radius or not 1 <= int(radius) <= TDK_DEFRINGE_MAX_SAMPLE_RADIUS:
            raise ValueError(f'radius must be an integer in 1..{TDK_DEFRINGE_MAX_SAMPLE_RADIUS}, got {radius}')
        strength = as_float32(strength)
        if not (math.isfinite(strength) and strength >= 0.0):
            raise ValueError(f'strength must be finite and >= 0 as a float32, got {strength}')
        floor = as_float32(floor)
        if not (math.isfinite(floor) and floor > 0.0):
            raise ValueError(f'floor must be finite and > 0 as a float32, got {floor}')
        if mode not in MODES:
            raise ValueError(f'mode must be one of {MODES}, got {mode!r}')
        if domain not in DOMAINS:
            raise ValueError(f'domain must be one of {DOMAINS}, got {domain!r}')
        self.radius, self.strength, self.floor, self.mode, self.domain = int(radius), strength, floor, mode, domain
        self._groups = 0   # a cap on the workgroups that gather the statistic (tests and measurements); 0: the library's
        self._prepare()

    @property
    def taps(self) -> tuple[float, ...]:
        """The blur's taps w0 .. wR as float32 values."""
        return self._taps.values

    @property
    def blur_radius(self) -> int:
        """R"""
        return self._taps.radius

    @property
    def launches(self) -> int:
        return 2

    @property
    def max_groups(self) -> int:
        """The most workgroups that gather the statistic."""
        return self._groups or TDK_DEFRINGE_MAX_GROUPS

    @max_groups.setter
    def max_groups(self, groups: int | None) -> None:
        """Cap the workgroups of the first launch (every cap gives the same bits: for tests and measurements); None: the library's."""
        groups = 0 if groups is None else int(groups)
        if not 0 <= groups <= TDK_DEFRINGE_MAX_GROUPS:
            raise ValueError(f'max_groups must be None or 1..{TDK_DEFRINGE_MAX_GROUPS}, got {groups}')
        self._groups = groups

    def _flags(self) -> int:
        return ((TDK_DEFRINGE_LINEAR if self.domain == 'linear' else 0) | (TDK_DEFRINGE_STATIC if self.mode == 'static' else 0)
                | (self._groups << TDK_DEFRINGE_GROUPS_SHIFT))

    def __repr__(self):
        return (f'Defringe({self.width}x{self.height}, {self._taps!r}, blur_radius={self.blur_radius}, radius={self.radius}, strength={self.strength:g}, '
                f'floor={self.floor:g}, mode={self.mode!r}, domain={self.domain!r})')

    def workspace_bytes(self) -> int:
        """Bytes of the plane of E and the partial sums between the two launches."""
        return int(lib.tdk_defringe_workspace_bytes(self.width, self.height))

    def lds_bytes(self, dtype: torch.dtype = torch.float32) -> int:
        """LDS one workgroup takes on frames of this type, the larger of the two launches (0: not a legal call)."""
        return int(lib.tdk_defringe_lds_bytes(TAGS.get(dtype, -1), self.blur_radius, self.radius, self._flags()))

    def _buffers(self, device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
        """(the record of S and th, the workspace): the two parts of the stream's buffer."""
        buf = self._workspace(device)
        return buf[:STATS_BYTES], buf[STATS_BYTES:]

    def _run(self, image: torch.Tensor, want_mask: bool, want_edge: bool):
        height, width, _, tag = self._float_frame(image, 'Defringe', 'image must have 3 channels')
        with torch.cuda.device(image.device):
            out = torch.empty_like(image)
            m = torch.empty((height, width), dtype=torch.uint8, device=image.device) if want_mask else None
            e = torch.empty((height, width), dtype=torch.float32, device=image.device) if want_edge else None
            stats, ws = self._buffers(image.device)
            rc = lib.tdk_defringe(_ptr(image), _ptr(out), _ptr(m), _ptr(e), _ptr(stats), _ptr(ws), width, height, tag, self._taps.c_array, self.blur_radius, self.radius,
                                  self.strength, self.floor, self._flags(), _stream())
        check(rc)
        return out, m, e

    def process(self, image: torch.Tensor, return_mask: bool = False):
        """(H, W, 3) float32 or float16 -> the defringed frame of the same type.  return_mask: (frame, m) with the (H, W) uint8 mask,
        1 where a pixel was rewritten."""
        out, m, _ = self._run(image, bool(return_mask), False)
        return (out, m) if return_mask else out

    def edge(self, image: torch.Tensor) -> torch.Tensor:
        """The (H, W) float32 edge chroma E alone (the frame is computed and dropped)."""
        return self._run(image, False, True)[2]

    def threshold(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(S, th) of the last call on the current stream: views of the device record, an int64 and a float32 scalar, valid in stream
        order and overwritten by the next call on this stream.  No synchronisation."""
        stats, _ = self._buffers(self._home_device())
        return stats[:8].view(torch.int64)[0], stats[8:12].view(torch.float32)[0]


__all__ = ['Defringe']
