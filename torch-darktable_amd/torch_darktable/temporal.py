"""Temporal denoiser (include/tdk_hip_temporal.h) -- a motion-adaptive recursive filter on raw Bayer mosaics, for frames that arrive
as a stream.

In a stream the cheapest noise reduction is the previous frames: a static site averaged over n frames loses a factor n of variance
and no detail.  `TemporalDenoise` keeps a running average and an effective frame count per site.  The squared difference between the
frame and the average, summed over a (2r + 1) x (2r + 1) window and divided by the variance the noise model predicts for it, tells
where the scene moved; there the count falls back to one and the average restarts from the frame.

    profile = NoiseProfile(device, (4096, 3072), BayerPattern.RGGB)
    model = profile.estimate(mosaic)
    temporal = TemporalDenoise(device, (4096, 3072), BayerPattern.RGGB, model, max_frames=8)
    for frame in camera:                      # (H, W) float32 or float16, the linear mosaic without white-balance gains
        mosaic = temporal.process(frame, key='left')

It acts on raw mosaics only, in front of the demosaic: there the noise of neighbouring sites is independent and the model
var(x) = a*x + b is exact.  The exact formulas are in the header; a NumPy restatement (tests/temporal_spec.py) predicts every bit of
the output and of the state.  One tile launch and a one-lane launch that advances the frame index, on PyTorch's current stream; no
atomics, no memset, no copy, no synchronisation.  Which of the two copies of the state a call reads is decided on the device by that
index, so a captured call can be replayed any number of times.  The twelve numbers of the noise model are read from device memory by
every call: an in-place update (a new `NoiseProfile.estimate` copied into `noise_model.model`) reaches a captured graph.
"""

from __future__ import annotations

import torch

from ._mosaic import FLOAT_TAGS, MosaicStage, check_gains, check_pattern, check_radius, check_storage, out_dtype_of, positive_float32, window_repr, window_thresholds
from ._native import TDK_TEMPORAL_HEAD_BYTES, TDK_TEMPORAL_MAX_FRAMES, TDK_TEMPORAL_TILE_H, TDK_TEMPORAL_TILE_W, check, lib
from ._stage import as_float32
from .bayer import BayerPattern
from .noiseprofile import NOISE_MODEL, NoiseModel
from .torch_darktable_extension import _pattern, _ptr, _require, _stream


class TemporalDenoise(MosaicStage):
    """Recursive temporal filter for (H, W) mosaics of one size; image_size is (width, height), both even.  `thresholds` = (t_lo, t_hi):
    a window whose difference energy is below t_lo times the predicted variance keeps its history, one above t_hi loses it, linear in
    between.  `pixel_threshold`: a site whose own difference exceeds that many predicted sigmas restarts whatever its window says (None:
    no such test).  `max_frames`: the largest effective frame count, 1..64.  `state_dtype`: the storage of the running average
    (float16 halves its traffic; the count is always binary16)."""

    TILE = (TDK_TEMPORAL_TILE_W, TDK_TEMPORAL_TILE_H)   # the output tile of a workgroup (csrc/temporal.hip)

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, noise_model: NoiseModel, radius: int = 2,
                 thresholds: tuple[float, float] = (1.5, 3.0), pixel_threshold: float | None = 4.0, max_frames: float = 8.0, variance_floor: float = 1e-12,
                 state_dtype: torch.dtype = torch.float32):
        super().__init__(device, image_size)
        check_pattern(bayer_pattern)
        self._check_even()
        check_radius(radius)
        self.thresholds, self.pixel_threshold, self._c2 = window_thresholds(thresholds, pixel_threshold)
        n_max = as_float32(max_frames)
        if not 1.0 <= n_max <= TDK_TEMPORAL_MAX_FRAMES:
            raise ValueError(f'max_frames must be in 1..{TDK_TEMPORAL_MAX_FRAMES}, got {max_frames}')
        v_min = positive_float32(variance_floor, 'variance_floor')
        if state_dtype not in FLOAT_TAGS:
            raise ValueError(f'state_dtype must be float32 or float16, got {state_dtype}')
        self.bayer_pattern, self.radius = bayer_pattern, int(radius)
        self.max_frames, self.variance_floor, self.state_dtype = n_max, v_min, state_dtype
        self.noise_model = noise_model
        self._states: dict = {}
        if torch.cuda.is_available():   # (an object can be built and queried without a GPU; nothing runs there)
            self.prepare([None])

    noise_model = NOISE_MODEL

    def __repr__(self):
        return (f'TemporalDenoise({self.width}x{self.height}, {self.bayer_pattern.name}, radius={self.radius}, {window_repr(self)}, '
                f'max_frames={self.max_frames:g}, state_dtype={self.state_dtype})')

    def lds_bytes(self) -> int:
        """Static LDS of a workgroup: the two staged planes and the two planes of row sums."""
        return int(lib.tdk_temporal_lds_bytes(self.radius))

    def state_bytes(self) -> int:
        """The state of one key: the head, two copies of the running average and two of the count."""
        return int(lib.tdk_temporal_state_bytes(self.width, self.height, FLOAT_TAGS[self.state_dtype]))

    def _plane_bytes(self) -> tuple[int, int]:
        sites = self.width * self.height
        align = lambda n: (n + 15) // 16 * 16
        return align(sites * (4 if self.state_dtype == torch.float32 else 2)), align(sites * 2)

    def prepare(self, keys) -> None:
        """Allocate and reset the state of every key that has none yet (ahead of a capture: `process` then allocates nothing)."""
        device = self._home_device()
        for key in keys:
            if key not in self._states:
                with torch.cuda.device(device):
                    self._states[key] = torch.empty(self.state_bytes(), dtype=torch.uint8, device=device)
                self._reset(self._states[key])

    def _reset(self, state: torch.Tensor) -> None:
        with torch.cuda.device(state.device):
            check(lib.tdk_temporal_reset(_ptr(state), _stream()))

    def reset(self, key=...) -> None:
        """Forget the history of one key, or of every key: the next frame passes through.  One one-lane launch per key on the current
        stream; the planes are not cleared."""
        if key is ...:
            for state in self._states.values():
                self._reset(state)
            return
        if key not in self._states:
            raise KeyError(f'TemporalDenoise has no state for key {key!r}')
        self._reset(self._states[key])

    def frames(self, key=None) -> torch.Tensor:
        """The index word of the key's state as a one-element device tensor (0: no history)."""
        return self._states[key][:4].view(torch.uint32)

    def state(self, key=None) -> tuple[torch.Tensor, torch.Tensor]:
        """(accumulated, count): views of the planes the next call will read, (H, W) each, state_dtype and float16.  Copies the index
        word to the host and waits for it.  With an index of 0 the planes are not trusted by the next call."""
        buf = self._states[key]
        plane = (int(self.frames(key).item()) + 1) & 1
        pa, pc = self._plane_bytes()
        sites, hw = self.width * self.height, (self.height, self.width)
        acc_at = TDK_TEMPORAL_HEAD_BYTES + plane * pa
        cnt_at = TDK_TEMPORAL_HEAD_BYTES + 2 * pa + plane * pc
        acc = buf[acc_at:acc_at + pa].view(self.state_dtype)[:sites].view(hw)
        cnt = buf[cnt_at:cnt_at + pc].view(torch.float16)[:sites].view(hw)
        return acc, cnt

    def _prepared(self, key) -> bool:
        return key in self._states

    def _begin(self, mosaic: torch.Tensor, key, gains, out_dtype) -> tuple[torch.dtype, torch.Tensor, torch.Tensor]:
        """The checks of `process` and the state of `key`, prepared here when it is not yet: (out_dtype, model, state)."""
        self._check_shape(mosaic)
        out_dtype = out_dtype_of(out_dtype, mosaic.dtype)
        check_storage(mosaic)
        model = self._noise_model.model
        _require(model.device == mosaic.device, 'The model must be on the device of the input')
        check_gains(gains, mosaic.device)
        if not self._prepared(key):
            self.prepare([key])
        state = self._states[key]
        _require(state.device == mosaic.device, 'The state must be on the device of the input')
        return out_dtype, model, state

    def process(self, mosaic: torch.Tensor, key=None, gains: torch.Tensor | None = None, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """The next frame of the sequence `key` -> the filtered frame, a fresh tensor.  The calls of one key must be ordered on one stream
        by the caller; different keys share nothing.  gains: a (3,) float32 device tensor, the white-balance gains the mosaic has been
        multiplied by since the model was measured.  A key first seen here is prepared here (an allocation: not inside a capture)."""
        out_dtype, model, state = self._begin(mosaic, key, gains, out_dtype)
        with torch.cuda.device(mosaic.device):
            out = torch.empty((self.height, self.width), dtype=out_dtype, device=mosaic.device)
            rc = lib.tdk_temporal_denoise(_ptr(mosaic), FLOAT_TAGS[mosaic.dtype], _ptr(out), FLOAT_TAGS[out_dtype], _ptr(state), FLOAT_TAGS[self.state_dtype], self.width,
                                          self.height, _pattern(self.bayer_pattern), _ptr(model), _ptr(gains), self.radius, self.thresholds[0],
                                          self.thresholds[1], self._c2, self.max_frames, self.variance_floor, _stream())
        check(rc)
        return out


__all__ = ['TemporalDenoise']
