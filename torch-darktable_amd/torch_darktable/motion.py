"""Motion estimation on raw Bayer mosaics and the motion-compensated temporal denoiser (include/tdk_hip_motion.h).

`TemporalDenoise` averages a mosaic over time per site and restarts where the frame differs from its running average.  That is right
for a static camera; when the whole frame pans by a few sites per frame every textured site restarts every frame.  `MotionEstimate`
finds one displacement per tile of the temporal filter (64 x 32 sites) by hierarchical block matching on an 8-bit grey pyramid of the
mosaic, and `MotionTemporalDenoise` is a `TemporalDenoise` that reads its history where the scene came from.

    me = MotionEstimate(device, (4096, 3072), levels=3, search=4)
    field = me.estimate(cur, ref)                   # (Ty, Tx, 2) int16, (dy, dx) in sites: ref[p + d] ~ cur[p]
    mt = MotionTemporalDenoise(device, (4096, 3072), BayerPattern.RGGB, model, motion=me, max_frames=8)
    for frame in camera:
        mosaic = mt.process(frame, key='left')      # pyramid, match, compensated filter, advance: four launches

Displacements are even numbers of sites, so the CFA colours of a site and of its history agree; the estimator is integer arithmetic
on the grey pyramid, so a NumPy restatement (tests/motion_spec.py) predicts every bit of the pyramid, the field, the costs, the output
and the state.  Everything is on PyTorch's current stream; no atomics, no memset, no copy, no synchronisation.  Which pyramid slot is
the previous frame's is decided on the device by the frame index of the temporal state, like the state's planes: a captured call can
be replayed any number of times.  It acts on raw mosaics only.
"""

from __future__ import annotations

import math

import torch

from ._mosaic import FLOAT_TAGS, MosaicStage
from ._native import TDK_MOTION_MAX_LEVELS, TDK_MOTION_MAX_SEARCH, TDK_MOTION_MAX_ZERO_BIAS, TDK_MOTION_TILE_H, TDK_MOTION_TILE_W, check, lib
from ._stage import as_float32
from .temporal import TemporalDenoise
from .torch_darktable_extension import _pattern, _ptr, _require, _stream

# The zero preference of tdk_motion_match in grey-level SAD units: twice the smallest bias at which every tile of 20 noisy frame pairs
# of the synthetic chart without motion came out zero, at two gains (DESIGN.md 3.15 has the measurement).
DEFAULT_ZERO_BIAS = 300


class MotionEstimate(MosaicStage):
    """Block-matching motion estimator for (H, W) mosaics of one size; image_size is (width, height), both even.  `levels` of the grey
    pyramid (1..4) and the `search` range of the coarsest level (1..4) give max_displacement = 2 * ((search + 1) * 2**(levels - 1) - 1)
    sites.  `zero_bias`: a tile moves only when the best match beats no motion by more than that many grey levels of summed absolute
    difference (0..65535).  `white_level`: the mosaic value that maps to the top of the grey range."""

    TILE = (TDK_MOTION_TILE_W, TDK_MOTION_TILE_H)

    def __init__(self, device: torch.device, image_size: tuple[int, int], levels: int = 3, search: int = 4, zero_bias: int = DEFAULT_ZERO_BIAS,
                 white_level: float = 1.0):
        super().__init__(device, image_size)
        self._check_even()
        if isinstance(levels, bool) or levels not in range(1, TDK_MOTION_MAX_LEVELS + 1):
            raise ValueError(f'levels must be an integer in 1..{TDK_MOTION_MAX_LEVELS}, got {levels}')
        if isinstance(search, bool) or search not in range(1, TDK_MOTION_MAX_SEARCH + 1):
            raise ValueError(f'search must be an integer in 1..{TDK_MOTION_MAX_SEARCH}, got {search}')
        if isinstance(zero_bias, bool) or not isinstance(zero_bias, int) or not 0 <= zero_bias <= TDK_MOTION_MAX_ZERO_BIAS:
            raise ValueError(f'zero_bias must be an integer in 0..{TDK_MOTION_MAX_ZERO_BIAS}, got {zero_bias}')
        white = as_float32(white_level)
        scale = as_float32(1.0 / (4.0 * white)) if math.isfinite(white) and white > 0.0 else math.nan
        if not (math.isfinite(scale) and scale > 0.0):
            raise ValueError(f'white_level must be finite and > 0 with a finite 1 / (4 white_level), got {white_level}')
        self.levels, self.search, self.zero_bias, self.white_level = int(levels), int(search), int(zero_bias), white
        self.scale = scale
        self._pyramids: dict = {}

    @property
    def tiles(self) -> tuple[int, int]:
        """(Ty, Tx): the shape of the field."""
        return (-(-self.height // TDK_MOTION_TILE_H), -(-self.width // TDK_MOTION_TILE_W))

    @property
    def max_displacement(self) -> int:
        return 2 * ((self.search + 1) * 2 ** (self.levels - 1) - 1)

    def __repr__(self):
        return (f'MotionEstimate({self.width}x{self.height}, levels={self.levels}, search={self.search}, zero_bias={self.zero_bias}, '
                f'white_level={self.white_level:g})')

    def pyramid_bytes(self) -> int:
        """A pyramid buffer: two slots of all levels."""
        return int(lib.tdk_motion_pyramid_bytes(self.width, self.height, self.levels))

    def level_sizes(self) -> list[tuple[int, int]]:
        """(rows, columns) of every level."""
        out, h, w = [], self.height // 2, self.width // 2
        for _ in range(self.levels):
            out.append((h, w))
            h, w = (h + 1) // 2, (w + 1) // 2
        return out

    def level_offsets(self) -> tuple[list[int], int]:
        """(byte offset of every level in its slot, bytes of a slot)."""
        at, total = [], 0
        for h, w in self.level_sizes():
            at.append(total)
            total += (h * w + 15) // 16 * 16
        return at, total

    def new_pyramid(self, device: torch.device) -> torch.Tensor:
        return torch.empty(self.pyramid_bytes(), dtype=torch.uint8, device=device)

    def new_field(self, device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
        """(field, costs) of one frame: (Ty, Tx, 2) int16 and (Ty, Tx, 2) uint32."""
        ty, tx = self.tiles
        return torch.empty((ty, tx, 2), dtype=torch.int16, device=device), torch.empty((ty, tx, 2), dtype=torch.int32, device=device).view(torch.uint32)

    def level(self, pyramid: torch.Tensor, slot: int, k: int) -> torch.Tensor:
        """A view of level k of one slot of a pyramid buffer, (rows, columns) uint8."""
        at, total = self.level_offsets()
        h, w = self.level_sizes()[k]
        start = slot * total + at[k]
        return pyramid[start:start + h * w].view(h, w)

    def build_pyramid(self, mosaic: torch.Tensor, pyramid: torch.Tensor, which: int, index: torch.Tensor | None = None) -> None:
        """One launch: the grey pyramid of `mosaic` into slot `which` of `pyramid`, or (index + which) & 1 with a device frame index."""
        self._check_mosaic(mosaic, 'input')
        with torch.cuda.device(mosaic.device):
            check(lib.tdk_motion_pyramid(_ptr(mosaic), FLOAT_TAGS[mosaic.dtype], self.width, self.height, self.scale, self.levels, _ptr(pyramid), _ptr(index), int(which),
                                         _stream()))

    def match(self, pyramid_cur: torch.Tensor, which_cur: int, pyramid_ref: torch.Tensor, which_ref: int, field: torch.Tensor, costs: torch.Tensor | None = None,
              index: torch.Tensor | None = None) -> None:
        """One launch: the displacement of every tile into `field` (and the costs into `costs`)."""
        with torch.cuda.device(field.device):
            check(lib.tdk_motion_match(_ptr(pyramid_cur), int(which_cur), _ptr(pyramid_ref), int(which_ref), self.width, self.height, self.levels, self.search,
                                       self.zero_bias, _ptr(index), _ptr(field), _ptr(costs), _stream()))

    def estimate(self, cur: torch.Tensor, ref: torch.Tensor, return_costs: bool = False):
        """The displacement of every tile of `cur` against `ref`: a fresh (Ty, Tx, 2) int16 tensor of (dy, dx) in sites with
        ref[p + d] ~ cur[p]; with return_costs also the (Ty, Tx, 2) uint32 costs (of the result, of no motion).  Three launches; the
        pyramid buffer is kept per device, so the calls of one object must be ordered on one stream by the caller."""
        self._check_mosaic(cur, 'cur')
        self._check_mosaic(ref, 'ref')
        _require(cur.device == ref.device, 'cur and ref must be on one device')
        if cur.device not in self._pyramids:
            with torch.cuda.device(cur.device):
                self._pyramids[cur.device] = self.new_pyramid(cur.device)
        pyramid = self._pyramids[cur.device]
        with torch.cuda.device(cur.device):
            field, costs = self.new_field(cur.device)
        self.build_pyramid(cur, pyramid, 0)
        self.build_pyramid(ref, pyramid, 1)
        self.match(pyramid, 0, pyramid, 1, field, costs)
        return (field, costs) if return_costs else field


class MotionTemporalDenoise(TemporalDenoise):
    """A `TemporalDenoise` whose history follows the scene: every frame is matched against the previous one per tile (`motion`, a
    `MotionEstimate` of the same image size) and the filter reads the running average and the count at the displaced site.  A history
    site outside the frame restarts.  The state is that of `TemporalDenoise`; the other arguments are its arguments."""

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern, noise_model, motion: MotionEstimate | None = None, **kwargs):
        if motion is None:
            motion = MotionEstimate(device, image_size)
        if not isinstance(motion, MotionEstimate):
            raise TypeError(f'motion must be a MotionEstimate, got {type(motion).__name__}')
        if motion.image_size != tuple(int(v) for v in image_size):
            raise ValueError(f'motion is for {motion.image_size}, the filter for {tuple(image_size)}')
        self.motion = motion
        self._buffers: dict = {}
        super().__init__(device, image_size, bayer_pattern, noise_model, **kwargs)

    def __repr__(self):
        return 'Motion' + super().__repr__()[:-1] + f', motion={self.motion!r})'

    def prepare(self, keys) -> None:
        """Allocate and reset the state of every key that has none yet, and its pyramid buffer, field and costs (ahead of a capture:
        `process` then allocates nothing but its output)."""
        keys = list(keys)
        super().prepare(keys)
        for key in keys:
            if key not in self._buffers:
                device = self._states[key].device
                with torch.cuda.device(device):
                    self._buffers[key] = (self.motion.new_pyramid(device), *self.motion.new_field(device))

    def _prepared(self, key) -> bool:
        return key in self._states and key in self._buffers

    def field(self, key=None) -> torch.Tensor:
        """The (Ty, Tx, 2) int16 displacements the last call of the key used: a device tensor the next call overwrites."""
        return self._buffers[key][1]

    def costs(self, key=None) -> torch.Tensor:
        """The (Ty, Tx, 2) uint32 costs (of the displacement used, of no motion) of the last call of the key."""
        return self._buffers[key][2]

    def process(self, mosaic: torch.Tensor, key=None, gains: torch.Tensor | None = None, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """The next frame of the sequence `key` -> the filtered frame, a fresh tensor: the pyramid of the frame into the slot of this
        frame index, the match against the other slot, the compensated filter, the advance.  Otherwise as `TemporalDenoise.process`."""
        out_dtype, model, state = self._begin(mosaic, key, gains, out_dtype)
        pyramid, field, costs = self._buffers[key]
        me = self.motion
        with torch.cuda.device(mosaic.device):
            out = torch.empty((self.height, self.width), dtype=out_dtype, device=mosaic.device)
            stream = _stream()
            # the first word of the state is the frame index: slot idx & 1 takes this frame, slot (idx + 1) & 1 holds the previous one
            check(lib.tdk_motion_pyramid(_ptr(mosaic), FLOAT_TAGS[mosaic.dtype], self.width, self.height, me.scale, me.levels, _ptr(pyramid), _ptr(state), 0, stream))
            check(lib.tdk_motion_match(_ptr(pyramid), 0, _ptr(pyramid), 1, self.width, self.height, me.levels, me.search, me.zero_bias, _ptr(state), _ptr(field),
                                       _ptr(costs), stream))
            check(lib.tdk_motion_temporal_denoise(_ptr(mosaic), FLOAT_TAGS[mosaic.dtype], _ptr(out), FLOAT_TAGS[out_dtype], _ptr(state), FLOAT_TAGS[self.state_dtype], self.width,
                                                  self.height, _pattern(self.bayer_pattern), _ptr(model), _ptr(gains), self.radius, self.thresholds[0],
                                                  self.thresholds[1], self._c2, self.max_frames, self.variance_floor, _ptr(field), stream))
        return out


__all__ = ['MotionEstimate', 'MotionTemporalDenoise']
