"""What the frame stages share on the host: float32 rounding, luminance weights, the taps of a separable blur, and the state of a
stage that is bound to one (width, height) -- ToneEqualizer, Dehaze, Deconvolve, Defringe; Sharpen and Filmic take the functions.
A stage is its formulas, its own checks and its kernel; the messages here are the ones those stages have always raised."""

from __future__ import annotations

import ctypes
import math

import torch

from ._frames import check_frame, check_size, require_cuda_device
from ._native import TDK_F16, TDK_F32, lib
from ._streams import StreamBuffers

REC709 = (0.2126, 0.7152, 0.0722)


def as_float32(value) -> float:
    """The float32 nearest to value, as a Python float: what the device will see."""
    return ctypes.c_float(float(value)).value


def luma_weights(weights) -> tuple[tuple[float, float, float], ctypes.Array]:
    """(the three luminance weights as float32 values, the same as a C array); None: Rec. 709."""
    weights = REC709 if weights is None else tuple(float(v) for v in weights)
    if len(weights) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in weights):
        raise ValueError(f'weights must be three finite values >= 0, got {weights}')
    values = tuple(as_float32(v) for v in weights)
    return values, (ctypes.c_float * 3)(*values)


def home_device(device: torch.device) -> torch.device:
    """The device an object built for `device` keeps its tensors on: 'cuda' without an index is the current one."""
    return torch.device('cuda', torch.cuda.current_device()) if device.index is None else device


class SeparableTaps:
    """The taps w0 .. wR of a symmetric separable blur as float32 values: immutable, from a Gaussian's sigma or a caller's values."""

    __slots__ = ('values', 'c_array', 'sigma', '_name')

    def __init__(self, values: tuple[float, ...], name: str, sigma: float | None):
        self.values, self._name, self.sigma = values, name, sigma
        self.c_array = (ctypes.c_float * len(values))(*values)

    @staticmethod
    def from_sigma(weights_fn, sigma: float, lo: float, hi: float, max_radius: int) -> 'SeparableTaps':
        """The taps the library makes of a Gaussian (weights_fn: its tdk_*_weights); sigma as the stage rounded it."""
        if not lo <= sigma <= hi:
            raise ValueError(f'sigma must lie in [{lo:g}, {hi:g}], got {sigma}')
        buf, radius = (ctypes.c_float * (max_radius + 1))(), ctypes.c_int(0)
        if weights_fn(sigma, buf, ctypes.byref(radius)) != 0:
            raise ValueError(lib.tdk_last_error().decode('utf-8', 'replace'))
        return SeparableTaps(tuple(buf[: radius.value + 1]), 'taps', sigma)

    @staticmethod
    def from_values(values, max_radius: int, name: str) -> 'SeparableTaps':
        """A caller's own taps, rounded to float32 and checked; `name` is the stage's word for them in its messages and its repr.
        Taps that are a SeparableTaps already are returned as they are."""
        if isinstance(values, SeparableTaps):
            return values
        values = tuple(as_float32(w) for w in values)
        if not 2 <= len(values) <= max_radius + 1:
            raise ValueError(f'{name} must hold 2..{max_radius + 1} values (radius 1..{max_radius}), got {len(values)}')
        if not all(math.isfinite(w) and w >= 0.0 for w in values):
            raise ValueError(f'{name} must be finite and >= 0, got {values}')
        return SeparableTaps(values, name, None)

    @property
    def radius(self) -> int:
        return len(self.values) - 1

    def __repr__(self):
        return f'sigma={self.sigma:g}' if self.sigma is not None else f'{self._name}={self.values}'


class FrameStage:
    """A stage on frames of one size (width, height) that keeps a workspace per stream.  A subclass gives workspace_bytes()."""

    _record_bytes = 0   # bytes a stage keeps in front of its workspace, in the same buffer

    def __init__(self, device: torch.device, image_size: tuple[int, int]):
        require_cuda_device(device)
        check_size('Image', image_size)
        self._device = device
        self.width, self.height = int(image_size[0]), int(image_size[1])
        self._workspaces = StreamBuffers()

    @property
    def image_size(self) -> tuple[int, int]:
        return (self.width, self.height)

    def workspace_bytes(self) -> int:
        raise NotImplementedError

    def _home_device(self) -> torch.device:
        return home_device(self._device)

    def _workspace(self, device: torch.device) -> torch.Tensor:
        """What the stage keeps between its launches, one buffer per stream: the object may be used from several streams at once.
        The buffer of the stream current at construction exists from then on, so a capture allocates nothing.  Every value read was
        written by the same call: the buffer is never cleared."""
        return self._workspaces.get(self._record_bytes + self.workspace_bytes(), device)

    def _prepare(self) -> torch.device | None:
        """Create the constructing stream's buffer and return the home device; None without a GPU (an object can be built and
        queried there; nothing runs)."""
        if not torch.cuda.is_available():
            return None
        where = self._home_device()
        self._workspace(where)
        return where

    def _float_frame(self, image: torch.Tensor, what: str, channels: str | None = None) -> tuple[int, int, int, int]:
        """(height, width, channels, dtype tag) of a float32 or float16 frame of the stage's size.  channels: the words that refuse
        a frame without three channels; None: one channel is taken too."""
        height, width, count, tag = check_frame(image, (self.height, self.width), what)
        if channels is not None and count != 3:
            raise ValueError(f'{channels}, got {count}')
        if tag not in (TDK_F32, TDK_F16):
            raise ValueError(f'image must be float32 or float16, got {image.dtype}')
        return height, width, count, tag
