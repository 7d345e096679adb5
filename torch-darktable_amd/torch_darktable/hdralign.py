"""Exposure brackets of a moving rig (include/tdk_hip_hdralign.h) -- the frames of a bracket are aligned per tile before the merge.

`HdrMerge` assumes that every frame of a bracket shows the same geometry: a frame that disagrees with a site's anchor loses its weight
there.  When the rig moves while it shoots, the frames are panned against each other by a few sites, every textured site disagrees, the
merge falls back to one frame, and where the anchor clips the site comes from a shorter frame that shows the scene somewhere else.
`MotionHdrMerge` is an `HdrMerge` that first matches every frame against the anchor frame per tile of 64 x 32 sites (`MotionEstimate`'s
block matching on grey pyramids, each frame brought into the units of the longest one) and then reads every frame where the scene is.

    merge = MotionHdrMerge(device, (4096, 3072), BayerPattern.RGGB, profile.estimate(mosaic))
    hdr = merge.process([long, mid, short], exposures=(1 / 30, 1 / 120, 1 / 480))   # in the coordinates of the anchor frame
    processor = ImageProcessor(..., hdr=merge)                                        # process_bracket then aligns before it merges

It acts on raw mosaics only.  Displacements are even numbers of sites, so the CFA colours of a site and of its displaced sample agree.
The exact formulas are in the header; a NumPy restatement (tests/hdralign_spec.py) predicts every bit of the output, every byte of the
mask and the pyramids and every integer of the fields and costs.  F pyramid launches, F - 1 match launches and one merge launch on
PyTorch's current stream, in sequence; no side streams, no atomics, no memset, no copy, no synchronisation.  With `fields` given it is
one launch.  The exposures and the noise model are read from device memory by every launch.
"""

from __future__ import annotations

import ctypes

import torch

from ._mosaic import FLOAT_TAGS
from ._native import check, lib
from ._streams import StreamBuffers
from .hdrmerge import HdrMerge
from .motion import MotionEstimate
from .torch_darktable_extension import _pattern, _ptr, _require, _stream

# The zero preference of the matches of this block in grey-level SAD units: twice the smallest bias at which every tile of 20 static
# noisy brackets of the synthetic chart came out zero, at exposure ratios 4 and 16 and scene gains 1 and 4 (DESIGN.md 3.23 has the
# measurement; tests/test_hdralign_spec.py holds the 20 values below it).  The frames of a bracket differ in noise after they are
# brought into common units, which is why this is not `motion.DEFAULT_ZERO_BIAS`.
DEFAULT_ZERO_BIAS = 750


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


class MotionHdrMerge(HdrMerge):
    """An `HdrMerge` whose frames follow the scene: every frame but the anchor frame `ref` is matched against it per tile (`motion`, a
    `MotionEstimate` of the same image size; default: one with this block's DEFAULT_ZERO_BIAS) and the merge reads frame f at the
    displacement of the output site's tile.  A displaced sample outside the frame counts as clipped.  The result lives in the
    coordinates of `ref`.  The other arguments are those of `HdrMerge`."""

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern, noise_model, motion: MotionEstimate | None = None, **kwargs):
        super().__init__(device, image_size, bayer_pattern, noise_model, **kwargs)
        if motion is None:
            motion = MotionEstimate(device, image_size, zero_bias=DEFAULT_ZERO_BIAS)
        if not isinstance(motion, MotionEstimate):
            raise TypeError(f'motion must be a MotionEstimate, got {type(motion).__name__}')
        if motion.image_size != self.image_size:
            raise ValueError(f'motion is for {motion.image_size}, the merge for {self.image_size}')
        self.motion = motion
        self._work = StreamBuffers()   # per frame count and stream: the pyramids, the fields and the costs; never cleared
        self._last = None              # (frame count, device) of the last call

    def __repr__(self):
        return 'Motion' + super().__repr__()[:-1] + f', motion={self.motion!r})'

    def lds_bytes(self) -> int:
        """Static LDS of a workgroup of the merge launch: that of `HdrMerge` and the displacements of the frames."""
        return int(lib.tdk_hdralign_lds_bytes(self.radius))

    # ---- workspace
    def _workspace(self, count: int, device: torch.device):
        """(pyramid buffers, fields (F, Ty, Tx, 2) int16, costs (F, Ty, Tx, 2) uint32) of the current stream."""
        me = self.motion
        ty, tx = me.tiles
        pyramid, buffers = _align16(me.pyramid_bytes()), (count + 1) // 2
        field_bytes, cost_bytes = _align16(count * ty * tx * 4), count * ty * tx * 8
        buf = self._work.get(buffers * pyramid + field_bytes + cost_bytes, device, key=count)
        pyramids = [buf[b * pyramid:b * pyramid + me.pyramid_bytes()] for b in range(buffers)]
        at = buffers * pyramid
        fields = buf[at:at + count * ty * tx * 4].view(torch.int16).view(count, ty, tx, 2)
        costs = buf[at + field_bytes:at + field_bytes + cost_bytes].view(torch.int32).view(torch.uint32).view(count, ty, tx, 2)
        return pyramids, fields, costs

    def prepare(self, num_frames: int, device: torch.device | None = None) -> None:
        """Allocate the workspace of brackets of `num_frames` frames on the current stream (ahead of a capture: `process` then
        allocates nothing but its output)."""
        if isinstance(num_frames, bool) or int(num_frames) != num_frames or not 2 <= num_frames <= self.MAX_FRAMES:
            raise ValueError(f'a bracket has 2..{self.MAX_FRAMES} frames, got {num_frames}')
        device = self._device if device is None else device
        with torch.cuda.device(device):
            self._workspace(int(num_frames), device)
        self._last = (int(num_frames), device)

    def _called(self):
        if self._last is None:
            raise RuntimeError('MotionHdrMerge: no bracket has been aligned yet (prepare, align or process come first)')
        return self._last

    def fields(self) -> torch.Tensor:
        """The (F, Ty, Tx, 2) int16 displacements (dy, dx) of the last call on the current stream: a device tensor the next call
        overwrites.  The row of the anchor frame is never written and never read."""
        return self._workspace(*self._called())[1]

    def costs(self) -> torch.Tensor:
        """The (F, Ty, Tx, 2) uint32 costs (of the displacement used, of no motion) of the last call on the current stream; the row of
        the anchor frame is never written."""
        return self._workspace(*self._called())[2]

    # ---- the steps
    @staticmethod
    def _resolve(exposures, ref, count: int) -> int:
        """The anchor frame: the host must know which frame the others are matched to."""
        if ref is not None:
            return int(ref)
        if isinstance(exposures, torch.Tensor):
            raise ValueError('ref=None needs exposures the host holds: with a device tensor of exposures pass the anchor frame as ref')
        hi = 0
        for f in range(1, count):   # the header's rule: the largest exposure, the lowest index
            if exposures[f] > exposures[hi]:
                hi = f
        return hi

    def _align(self, frames, exp: torch.Tensor, ref: int):
        """F pyramid launches and F - 1 match launches on the current stream; returns the fields."""
        me, count, first = self.motion, len(frames), frames[0]
        pyramids, fields, costs = self._workspace(count, first.device)
        self._last = (count, first.device)
        stream = _stream()
        for f, frame in enumerate(frames):
            check(lib.tdk_hdralign_pyramid(_ptr(frame), FLOAT_TAGS[frame.dtype], self.width, self.height, me.scale, me.levels, _ptr(pyramids[f // 2]), f % 2, _ptr(exp),
                                           count, f, stream))
        for f in range(count):
            if f != ref:   # cur: the anchor frame; ref of the match: frame f, so that frame_f[p + d] ~ anchor[p]
                check(lib.tdk_motion_match(_ptr(pyramids[ref // 2]), ref % 2, _ptr(pyramids[f // 2]), f % 2, self.width, self.height, me.levels, me.search,
                                           me.zero_bias, None, _ptr(fields[f]), _ptr(costs[f]), stream))
        return fields

    def align(self, frames, exposures, ref: int | None = None) -> torch.Tensor:
        """The displacements of a bracket against its anchor frame: `fields()` of this call, (F, Ty, Tx, 2) int16 with
        frame_f[p + d] ~ anchor[p].  2 F - 1 launches."""
        self._resolve(exposures, ref, 0)
        frames, exposures, _, _ = self._arguments(frames, exposures, ref, None)
        ref = self._resolve(exposures, ref, len(frames))
        with torch.cuda.device(frames[0].device):
            return self._align(frames, self._exposure_tensor(exposures, frames[0].device), ref)

    def process(self, frames, exposures, ref: int | None = None, out_dtype: torch.dtype | None = None, return_mask: bool = False,
                fields: torch.Tensor | None = None):
        """`HdrMerge.process` with every frame read where the scene is.  fields: None (the frames are matched against the anchor frame:
        2 F launches in all) or an (F, Ty, Tx, 2) int16 device tensor of displacements (one launch); odd values are masked and any value
        is memory-safe.  ref=None is the longest exposure, resolved on the host: with a device tensor of exposures ref must be given."""
        self._resolve(exposures, ref, 0)   # (refuses ref=None with exposures on the device before anything else is looked at)
        frames = self._frames(frames)
        count, (ty, tx) = len(frames), self.motion.tiles
        if fields is not None:
            _require(isinstance(fields, torch.Tensor) and tuple(fields.shape) == (count, ty, tx, 2) and fields.dtype == torch.int16 and fields.is_contiguous(),
                     f'fields must be a contiguous ({count}, {ty}, {tx}, 2) int16 tensor')
        frames, exposures, out_dtype, model = self._arguments(frames, exposures, ref, out_dtype)
        first = frames[0]
        ref = self._resolve(exposures, ref, count)
        if fields is not None:
            _require(fields.device == first.device, 'fields must be on the device of the frames')
        shape = (self.height, self.width)
        with torch.cuda.device(first.device):
            exp = self._exposure_tensor(exposures, first.device)
            if fields is None:
                fields = self._align(frames, exp, ref)
            out = torch.empty(shape, dtype=out_dtype, device=first.device)
            mask = torch.empty(shape, dtype=torch.uint8, device=first.device) if return_mask else None
            pointers = (ctypes.c_void_p * count)(*[frame.data_ptr() for frame in frames])
            rc = lib.tdk_hdralign_merge(pointers, count, FLOAT_TAGS[first.dtype], _ptr(out), FLOAT_TAGS[out_dtype], _ptr(mask), self.width, self.height,
                                        _pattern(self.bayer_pattern), _ptr(exp), ref, _ptr(model), self.radius, self.clip, self.thresholds[0],
                                        self.thresholds[1], self._c2, self.variance_floor, _ptr(fields), _stream())
        check(rc)
        return (out, mask) if return_mask else out


__all__ = ['MotionHdrMerge']
