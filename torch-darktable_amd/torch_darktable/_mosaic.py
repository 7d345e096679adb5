"""What the stages on raw (H, W) Bayer mosaics share on the host: the float dtype tags, the checks of a size, a pattern and whole CFA
cells, the window statistic of TemporalDenoise and HdrMerge, the filter of a frame and of a set of frames, and the state of a stage
bound to one (width, height) -- RawPrepare, Highlights, ChromaticAberration, NoiseProfile, TemporalDenoise, MotionEstimate, HdrMerge
and FrameStats.  Every check is a piece a constructor calls in its own order; the messages are the ones the stages have always raised."""

from __future__ import annotations

import math

import torch

from ._frames import MAX_SIZE, require_cuda_device
from ._native import TDK_F16, TDK_F32
from ._stage import as_float32, home_device
from ._streams import StreamBuffers
from .bayer import BayerPattern
from .torch_darktable_extension import _require

FLOAT_TAGS = {torch.float32: TDK_F32, torch.float16: TDK_F16}


def check_pattern(bayer_pattern) -> None:
    if not isinstance(bayer_pattern, BayerPattern):
        raise ValueError(f'Invalid bayer pattern: {bayer_pattern}')


def check_radius(radius) -> None:
    if radius not in (2, 3) or isinstance(radius, bool):
        raise ValueError(f'radius must be 2 or 3, got {radius}')


def positive_float32(value, name: str) -> float:
    """`value` as float32, finite and > 0 there; the message shows the caller's value."""
    rounded = as_float32(value)
    if not (math.isfinite(rounded) and rounded > 0.0):
        raise ValueError(f'{name} must be finite and > 0, got {value}')
    return rounded


def window_thresholds(thresholds, pixel_threshold) -> tuple[tuple[float, float], float | None, float]:
    """((t_lo, t_hi), pixel_threshold or None, c2) as float32 values; c2 is the squared pixel threshold the kernel compares with."""
    if len(tuple(thresholds)) != 2:
        raise ValueError(f'thresholds must be (t_lo, t_hi), got {thresholds}')
    t_lo, t_hi = (as_float32(v) for v in thresholds)
    if not (math.isfinite(t_lo) and math.isfinite(t_hi) and 0.0 < t_lo < t_hi and math.isfinite(as_float32(1.0 / as_float32(t_hi - t_lo)))):
        raise ValueError(f'thresholds must be finite with 0 < t_lo < t_hi, got {tuple(thresholds)}')
    if pixel_threshold is None:
        return (t_lo, t_hi), None, math.inf
    p = as_float32(pixel_threshold)
    c2 = as_float32(p * p)
    if not (math.isfinite(p) and p > 0.0 and c2 > 0.0):
        raise ValueError(f'pixel_threshold must be finite and > 0, or None, got {pixel_threshold}')
    return (t_lo, t_hi), p, c2


def window_repr(stage) -> str:
    pixel = stage.pixel_threshold
    return f'thresholds=({stage.thresholds[0]:g}, {stage.thresholds[1]:g}), pixel_threshold={pixel if pixel is None else format(pixel, "g")}'


def out_dtype_of(out_dtype, default: torch.dtype) -> torch.dtype:
    """The out_dtype rule: None is the input's type; float32 or float16."""
    out_dtype = default if out_dtype is None else out_dtype
    if out_dtype not in FLOAT_TAGS:
        raise ValueError(f'out_dtype must be float32 or float16, got {out_dtype}')
    return out_dtype


def check_storage(mosaic: torch.Tensor, tags=FLOAT_TAGS, kinds: str = 'float32 or float16') -> None:
    _require(mosaic.is_cuda, 'Input must be on CUDA device')
    _require(mosaic.is_contiguous(), 'Input must be contiguous')
    _require(mosaic.dtype in tags, f'Input tensor must be {kinds}')


def check_frame_set(frames) -> None:
    """The frames of a bracket or of an estimate: each on the device and contiguous, all of the first one's float type and device."""
    first = frames[0]
    for frame in frames:
        _require(frame.is_cuda, 'Input must be on CUDA device')
        _require(frame.is_contiguous(), 'Input must be contiguous')
        _require(frame.dtype in FLOAT_TAGS and frame.dtype == first.dtype, 'Input tensors must be all float32 or all float16')
        _require(frame.device == first.device, 'The frames must be on one device')


def check_gains(gains, device: torch.device) -> None:
    """The white-balance gains a mosaic has been multiplied by since its noise model was measured: None or a (3,) float32 tensor."""
    if gains is not None:
        _require(isinstance(gains, torch.Tensor) and tuple(gains.shape) == (3,) and gains.dtype == torch.float32 and gains.is_contiguous(),
                 'gains must be a contiguous (3,) float32 tensor')
        _require(gains.device == device, 'gains must be on the device of the input')


class MosaicStage:
    """A stage on (H, W) mosaics of one size; image_size is (width, height), each min_size..65535.  The pattern and the whole-cell
    check follow in the subclass, in its order."""

    def __init__(self, device: torch.device, image_size: tuple[int, int], min_size: int = 2):
        require_cuda_device(device)
        width, height = (int(v) for v in image_size)
        if not (min_size <= width <= MAX_SIZE and min_size <= height <= MAX_SIZE):
            raise ValueError(f'Image dimensions must be {min_size}..{MAX_SIZE}, got {width}x{height}')
        self._device = device
        self.width, self.height = width, height

    def _check_even(self, first_word: str = 'Mosaic') -> None:
        if self.width % 2 or self.height % 2:
            raise ValueError(f'{first_word} dimensions must be even (whole CFA cells), got {self.width}x{self.height}')

    @property
    def image_size(self) -> tuple[int, int]:
        return (self.width, self.height)

    def _home_device(self) -> torch.device:
        return home_device(self._device)

    def _keep_workspace(self) -> None:
        """For a stage whose workspace_bytes() is fixed at construction: the size is asked once, and the buffer of the stream current
        now exists from here on, so a capture allocates nothing (an object can be built and queried without a GPU; nothing runs there)."""
        self._workspace_bytes = self.workspace_bytes()
        self._workspaces = StreamBuffers()
        if torch.cuda.is_available():
            self._workspace(self._home_device())

    def _workspace(self, device: torch.device) -> torch.Tensor:
        """The records of the gather launch, one buffer per stream: the object may be used from several streams at once.  Every record
        a call reads it has written: the buffer is never cleared."""
        return self._workspaces.get(self._workspace_bytes, device)

    def _check_shape(self, mosaic: torch.Tensor, what: str = 'input') -> None:
        if tuple(mosaic.shape) != (self.height, self.width):
            raise RuntimeError(f'{type(self).__name__} {what} shape {tuple(mosaic.shape)} != expected {(self.height, self.width)}')

    def _check_mosaic(self, mosaic: torch.Tensor, what: str = 'input', tags=FLOAT_TAGS, kinds: str = 'float32 or float16') -> None:
        """_check_shape and check_storage, written out: a call of a small kernel is bound by the host."""
        if tuple(mosaic.shape) != (self.height, self.width):
            raise RuntimeError(f'{type(self).__name__} {what} shape {tuple(mosaic.shape)} != expected {(self.height, self.width)}')
        _require(mosaic.is_cuda, 'Input must be on CUDA device')
        _require(mosaic.is_contiguous(), 'Input must be contiguous')
        _require(mosaic.dtype in tags, f'Input tensor must be {kinds}')
