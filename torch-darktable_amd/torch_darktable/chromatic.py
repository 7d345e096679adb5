"""Lateral chromatic aberration (include/tdk_hip_ca.h) -- the lens magnifies red and blue a little differently from green, so that
towards the corners of a frame the three colour planes are 0.5 to 3 sites apart.  `ChromaticAberration` fits that to frames of the
camera and resamples the red and the blue plane of a raw mosaic back onto the green one:

    ca = ChromaticAberration(device, (4096, 3072), BayerPattern.RGGB)
    ca = ca.estimate(mosaics, noise_model=profile.estimate(mosaics))     # a new object; its model is a device tensor, nothing waits
    aligned = ca.correct(mosaic)                                          # green untouched, red and blue interpolated in their planes
    ca = ChromaticAberration.from_coefficients(device, (4096, 3072), BayerPattern.RGGB, red=(1.0004, 0, 0.0002), blue=(0.9997, 0, 0))

It acts on raw mosaics only, in front of the white balance and the demosaic: a demosaic reads misaligned planes as edges and mixes the
damage into all three channels, where a warp per channel can no longer undo it.  The model is lensfun's poly3 TCA model, the captured
radius as a function of the ideal one: s = v + c*rho + b*rho^2 per colour, with rho the distance from the optical centre over `rn`.
The exact formulas are in the header; a NumPy restatement (tests/chromatic_spec.py) predicts every bit of `correct`, every integer of
the workspace and every bit of the model of `estimate`.  `correct` is one tile launch; `estimate` one gather launch per frame and one
finishing launch, on PyTorch's current stream; no atomics on global memory, no memset, no copy, no synchronisation.  The model and the
noise model are read from device memory by every call: an `estimate` earlier on the stream feeds a captured `correct`.  The workspace
belongs to the object, one per stream, and is never cleared.
"""

from __future__ import annotations

import copy
import ctypes
import math

import torch

from ._mosaic import FLOAT_TAGS, MosaicStage, check_frame_set, check_pattern, check_storage, out_dtype_of
from ._native import (TDK_CA_BICUBIC, TDK_CA_BILINEAR, TDK_CA_LINEAR, TDK_CA_MAX_FRAMES, TDK_CA_MAX_SHIFT, TDK_CA_POLY3, TDK_CA_SUMS, TDK_CA_TILE_H, TDK_CA_TILE_W,
                      check, lib)
from ._stage import as_float32 as _f32
from ._streams import StreamBuffers
from .bayer import BayerPattern
from .noiseprofile import NoiseModel
from .torch_darktable_extension import _pattern, _ptr, _require, _stream

_INTERPS = {'bilinear': TDK_CA_BILINEAR, 'bicubic': TDK_CA_BICUBIC}
_FITS = {'linear': TDK_CA_LINEAR, 'poly3': TDK_CA_POLY3}


class ChromaticAberration(MosaicStage):
    """The model of one camera and the two operations on it; image_size is (width, height), both even.  `model`: a contiguous (2, 4)
    float32 tensor, rows red and blue, columns v, c, b, valid (None: the identity, created on first use on the device of the input);
    `center`: the optical centre (x0, y0) in site coordinates, None: ((W-1)/2, (H-1)/2); `rn`: the radius at which rho is 1, None: the
    distance from the centre to the farthest corner; `interp`: 'bilinear' or 'bicubic' (the Keys kernel with A = -0.75 of `Warp` and OpenCV).
    Bilinear is the default on evidence: the bicubic kernel does not reproduce a linear ramp, its position error reaches 0.1 site, and on
    the chart of tests/test_chromatic_spec.py it leaves a residual aberration of 0.13 site where bilinear leaves 0.02."""

    TILE = (TDK_CA_TILE_W, TDK_CA_TILE_H)   # the output tile of a workgroup of `correct` (csrc/cacorrect.hip)
    MAX_SHIFT = TDK_CA_MAX_SHIFT            # the largest displacement per axis, in sites
    MAX_FRAMES = TDK_CA_MAX_FRAMES

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, model: torch.Tensor | None = None,
                 center: tuple[float, float] | None = None, rn: float | None = None, interp: str = 'bilinear'):
        super().__init__(device, image_size)
        check_pattern(bayer_pattern)
        self._check_even()
        width, height = self.width, self.height
        if interp not in _INTERPS:
            raise ValueError(f"interp must be 'bilinear' or 'bicubic', got {interp!r}")
        if center is None:
            center = ((width - 1) / 2, (height - 1) / 2)
        if len(tuple(center)) != 2:
            raise ValueError(f'center must be (x0, y0), got {center}')
        x0, y0 = (_f32(v) for v in center)
        if not (math.isfinite(x0) and math.isfinite(y0)):
            raise ValueError(f'center must be finite, got {tuple(center)}')
        if rn is None:
            rn = math.hypot(max(x0, width - 1 - x0), max(y0, height - 1 - y0))
        rn = _f32(rn)
        if not (math.isfinite(rn) and rn > 0.0):
            raise ValueError(f'rn must be finite and > 0, got {rn}')
        if model is not None:
            self._check_model(model)
        self.bayer_pattern = bayer_pattern
        self.center, self.rn, self.interp = (x0, y0), rn, interp
        self._model = model
        self._workspaces = StreamBuffers()   # of `estimate`, per block size and stream; shared with the objects `estimate` returns
        if torch.cuda.is_available():   # (an object can be built and queried without a GPU; nothing runs there)
            self._workspace(64, self._home_device())

    @staticmethod
    def _check_model(model) -> None:
        if not isinstance(model, torch.Tensor) or tuple(model.shape) != (2, 4) or model.dtype != torch.float32 or not model.is_contiguous():
            raise ValueError(f'model must be a contiguous (2, 4) float32 tensor, got {tuple(getattr(model, "shape", ()))} {getattr(model, "dtype", type(model).__name__)}')

    @property
    def model(self) -> torch.Tensor | None:
        return self._model

    @model.setter
    def model(self, model: torch.Tensor | None) -> None:
        if model is not None:
            self._check_model(model)
        self._model = model

    def __repr__(self):
        return (f'ChromaticAberration({self.width}x{self.height}, {self.bayer_pattern.name}, center=({self.center[0]:g}, {self.center[1]:g}), rn={self.rn:g}, '
                f'interp={self.interp})')

    @staticmethod
    def _coefficients(values, what: str) -> tuple[float, float, float]:
        values = tuple(_f32(v) for v in values)
        if len(values) != 3 or not all(math.isfinite(v) for v in values):
            raise ValueError(f'{what} must be three finite values (v, c, b), got {values}')
        return values

    @classmethod
    def from_coefficients(cls, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, red=(1.0, 0.0, 0.0), blue=(1.0, 0.0, 0.0),
                          **kwargs) -> 'ChromaticAberration':
        """A known model, for instance the vr, cr, br / vb, cb, bb of a lens database with its own `rn`; the tensor is made on `device`."""
        red, blue = cls._coefficients(red, 'red'), cls._coefficients(blue, 'blue')
        self = cls(device, image_size, bayer_pattern, **kwargs)   # (the arguments are checked before anything touches the device)
        self._model = torch.tensor([[*red, 1.0], [*blue, 1.0]], dtype=torch.float32, device=device)
        return self

    @classmethod
    def identity(cls, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, **kwargs) -> 'ChromaticAberration':
        return cls.from_coefficients(device, image_size, bayer_pattern, **kwargs)

    def with_model(self, model: torch.Tensor) -> 'ChromaticAberration':
        """The same camera and host parameters around another model tensor."""
        self._check_model(model)
        other = copy.copy(self)
        other._model = model
        return other

    def lds_bytes(self, src_dtype: torch.dtype = torch.float32) -> int:
        """Static LDS of a workgroup of `correct`: the staged source box."""
        return int(lib.tdk_ca_lds_bytes(_INTERPS[self.interp], FLOAT_TAGS.get(src_dtype, -1)))

    def workspace_bytes(self, block: int = 64) -> int:
        return int(lib.tdk_ca_workspace_bytes(self.width, self.height, int(block)))

    def _workspace(self, block: int, device: torch.device) -> torch.Tensor:
        """One buffer per block size and stream.  That of the default block and of the stream current at construction exists from then
        on, so a capture allocates nothing.  Every record a call reads it has written: the buffer is never cleared."""
        return self._workspaces.get(self.workspace_bytes(block), device, key=block)

    def _model_of(self, model, device: torch.device) -> torch.Tensor:
        if isinstance(model, ChromaticAberration):
            model = model.model
        if model is None:
            model = self._model
        if model is None:   # the identity, made once (not inside a capture: build the object with a model for that)
            model = self._model = torch.tensor([[1.0, 0.0, 0.0, 1.0]] * 2, dtype=torch.float32, device=device)
        self._check_model(model)
        _require(model.device == device, 'The model must be on the device of the input')
        return model

    def _check_frame(self, frame, what: str) -> None:
        shape = (self.height, self.width)
        if not isinstance(frame, torch.Tensor) or tuple(frame.shape) != shape:
            raise RuntimeError(f'ChromaticAberration {what} shape {tuple(getattr(frame, "shape", ()))} != expected {shape}')

    def correct(self, mosaic: torch.Tensor, model=None, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """An (H, W) mosaic, float32 or float16, contiguous -> a fresh tensor: green as it is, red and blue taken from where the model
        says they were captured.  model: a (2, 4) tensor or a ChromaticAberration; None: the object's own."""
        self._check_frame(mosaic, 'input')
        out_dtype = out_dtype_of(out_dtype, mosaic.dtype)
        check_storage(mosaic)
        with torch.cuda.device(mosaic.device):
            model = self._model_of(model, mosaic.device)
            out = torch.empty(mosaic.shape, dtype=out_dtype, device=mosaic.device)
            rc = lib.tdk_ca_correct(_ptr(mosaic), FLOAT_TAGS[mosaic.dtype], _ptr(out), FLOAT_TAGS[out_dtype], self.width, self.height, _pattern(self.bayer_pattern),
                                    _ptr(model), self.center[0], self.center[1], self.rn, _INTERPS[self.interp], _stream())
        check(rc)
        return out

    def _frames(self, mosaics) -> list[torch.Tensor]:
        frames = [mosaics] if isinstance(mosaics, torch.Tensor) and mosaics.ndim == 2 else list(mosaics)
        if not 1 <= len(frames) <= TDK_CA_MAX_FRAMES:
            raise ValueError(f'estimate takes 1..{TDK_CA_MAX_FRAMES} frames, got {len(frames)}')
        for frame in frames:
            self._check_frame(frame, 'input')
        return frames

    @staticmethod
    def _estimate_arguments(noise_model, fit, clip, block, max_shift):
        if noise_model is not None and not isinstance(noise_model, NoiseModel):
            raise TypeError(f'noise_model must be a NoiseModel or None, got {type(noise_model).__name__}')
        if fit not in _FITS:
            raise ValueError(f"fit must be 'linear' or 'poly3', got {fit!r}")
        clip = _f32(clip)
        if not (math.isfinite(clip) and clip > 0.0):
            raise ValueError(f'clip must be finite and > 0, got {clip}')
        if isinstance(block, bool) or int(block) != block or not 16 <= int(block) <= 256 or int(block) % 2:
            raise ValueError(f'block must be an even integer in 16..256, got {block}')
        max_shift = _f32(max_shift)
        if not (math.isfinite(max_shift) and 0.0 < max_shift <= TDK_CA_MAX_SHIFT):
            raise ValueError(f'max_shift must be in (0, {TDK_CA_MAX_SHIFT}], got {max_shift}')
        return clip, int(block), max_shift

    def _run(self, mosaics, noise_model, fit, clip, block, max_shift) -> tuple[torch.Tensor, torch.Tensor]:
        """(model, workspace)"""
        frames = self._frames(mosaics)
        clip, block, max_shift = self._estimate_arguments(noise_model, fit, clip, block, max_shift)
        first = frames[0]
        check_frame_set(frames)
        noise = None if noise_model is None else noise_model.model
        if noise is not None:
            _require(noise.device == first.device, 'The noise model must be on the device of the input')
        pointers = (ctypes.c_void_p * len(frames))(*(frame.data_ptr() for frame in frames))
        with torch.cuda.device(first.device):
            workspace = self._workspace(block, first.device)
            model = torch.empty((2, 4), dtype=torch.float32, device=first.device)
            rc = lib.tdk_ca_estimate(pointers, len(frames), FLOAT_TAGS[first.dtype], self.width, self.height, _pattern(self.bayer_pattern), _ptr(noise), _FITS[fit],
                                     clip, block, max_shift, self.center[0], self.center[1], self.rn, _ptr(workspace), _ptr(model), _stream())
        check(rc)
        return model, workspace

    def estimate(self, mosaics, noise_model: NoiseModel | None = None, fit: str = 'linear', clip: float = 0.95, block: int = 64,
                 max_shift: float = 2.0) -> 'ChromaticAberration':
        """1 to 16 mosaics of the camera (a tensor or a list, all float32 or all float16) -> the fitted model around this object's host
        parameters.  Green gradients steer the fit: per block of `block` x `block` sites red and blue are regressed on green and its
        two derivatives, and a radial polynomial is fitted through the block displacements.  noise_model: the sensor's noise, without
        which the shift of a noisy frame comes out too small by a factor of three.  fit: 'linear' (v alone) or 'poly3' (v, c, b).  A
        sample at or above `clip` is left out with the sites that touch it; a block whose displacement exceeds `max_shift` is dropped.
        A frame that determines nothing gives rows with valid == 0, the identity."""
        model, _ = self._run(mosaics, noise_model, fit, clip, block, max_shift)
        return self.with_model(model)

    def statistics(self, mosaics, clip: float = 0.95, block: int = 64) -> torch.Tensor:
        """The integer block the model is derived from: (block rows, block columns, 2, 17) int64, a view of the workspace of the current
        stream (the next `estimate` on it overwrites it)."""
        _, workspace = self._run(mosaics, None, 'linear', clip, block, 2.0)
        nby, nbx = self.height // int(block), self.width // int(block)
        return workspace[:nby * nbx * 2 * TDK_CA_SUMS * 8].view(torch.int64).view(nby, nbx, 2, TDK_CA_SUMS)

    def refine(self, mosaics, model=None, **kwargs) -> 'ChromaticAberration':
        """model + estimate(correct(mosaics, model)) - identity: the fit is a linearisation, and what it leaves of a large aberration
        one more round finds.  Torch operations on the device coefficients; a residual that could not be fitted changes nothing."""
        frames = self._frames(mosaics)
        base = self._model_of(model, frames[0].device)
        residual = self.estimate([self.correct(frame, base) for frame in frames], **kwargs).model
        identity = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float32, device=base.device)
        refined = base.clone()
        refined[:, :3] += (residual[:, :3] - identity) * residual[:, 3:4]
        return self.with_model(refined)


__all__ = ['ChromaticAberration']
