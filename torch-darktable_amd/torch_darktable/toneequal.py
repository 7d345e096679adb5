"""Tone equalizer (include/tdk_hip_toneeq.h: tdk_toneeq) -- dodge and burn by exposure band, the stage darktable calls tone equalizer.

Every pixel is multiplied by a gain that depends on the brightness of the REGION it lies in, not on its own value: shadows come up,
highlights come down, and the texture inside a region keeps its contrast.  The region's brightness is the mask

    Y    = max(w . rgb, 0)                        luminance, Rec. 709 weights by default
    L    = mean of Y over cells of `cell` x `cell` pixels
    a, b = self-guided filter of L (He et al.): box windows of (2*radius + 1)^2 cells, a = var / (var + eps), b = mean - a*mean
    m    = up(box(a)) * Y + up(box(b))            bilinear between cell centres

and the gain is 2 ** correction(log2(m) + mask_exposure), looked up in a table of 32 nodes per octave over -16 .. 4 EV.  The correction
is darktable's: nine bands centred at -8 .. 0 EV (0 EV is a luminance of 1), Gaussians of sigma sqrt(2) whose weights are solved so
that the curve passes through the nine gains given.  The curve and the table are made on the host in float64 (nothing on the
device); the exact float32 formulas of the device are in the header, and a NumPy restatement (tests/toneequal_spec.py) predicts the
bits.  Three launches on PyTorch's current stream, no synchronisation; the workspace belongs to the object, one per stream:
capturable in a HIP graph from the first call, and bit-reproducible.

    te = ToneEqualizer(device, (4096, 3072), gains_ev=(3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0))     # lift the shadows by three stops
    out = te.process(rgb)                          # (H, W, 3) float32 or float16, the same type out; not clamped
    te.set_gains((0,) * 9)                         # a new table in the same device tensor: a captured process follows it
"""

from __future__ import annotations

import math

import numpy as np
import torch

from ._frames import TAGS
from ._native import TDK_TONEEQ_EV_MAX, TDK_TONEEQ_EV_MIN, TDK_TONEEQ_MAX_RADIUS, TDK_TONEEQ_STEPS, TDK_TONEEQ_TABLE, check, lib
from ._stage import FrameStage, as_float32, luma_weights
from .torch_darktable_extension import _ptr, _stream

CENTRES = tuple(float(c) for c in range(-8, 1))   # the nine bands, in EV
CELLS = (2, 4, 8, 16)
MAX_OVERSHOOT_EV = 1.0   # how far the curve may leave the range of its nodes between them


class ToneEqualizer(FrameStage):
    """Dodge and burn (H, W, 3) frames of one size (width, height).  gains_ev: nine gains in EV for the bands at -8 .. 0 EV;
    mask_exposure: EV added to the mask in front of the curve (places the frame's tones on the bands)."""

    TILE = (128, 32)  # (width, height) of one workgroup's tile in the apply launch (csrc/toneequal.hip: TE_TW, TE_TH)

    def __init__(self, device: torch.device, image_size: tuple[int, int], gains_ev=(0,) * 9, cell: int = 8, radius: int = 4, eps: float = 1e-4,
                 mask_exposure: float = 0.0, sigma: float = 2 ** 0.5, weights=None):
        super().__init__(device, image_size)
        if cell not in CELLS:
            raise ValueError(f'cell must be one of {CELLS}, got {cell}')
        if int(radius) != radius or not 0 <= int(radius) <= TDK_TONEEQ_MAX_RADIUS:
            raise ValueError(f'radius must be an integer in 0..{TDK_TONEEQ_MAX_RADIUS}, got {radius}')
        eps = as_float32(eps)
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError(f'eps must be finite and > 0 as a float32, got {eps}')
        self.weights, self._c_weights = luma_weights(weights)
        if not (math.isfinite(float(sigma)) and float(sigma) > 0.0):
            raise ValueError(f'sigma must be finite and > 0, got {sigma}')
        self.cell, self.radius, self.eps, self.sigma = int(cell), int(radius), eps, float(sigma)
        self._gains_ev, self.mask_exposure = self._check_gains(gains_ev, mask_exposure)
        # the table on the host, kept by the object: set_gains fills it and copies it to the device in stream order
        self._host_table = torch.from_numpy(self.make_table(self._gains_ev, self.mask_exposure, self.sigma))
        where = self._prepare()
        self._table: torch.Tensor | None = None if where is None else self._host_table.to(where)

    # ---- the curve, on the host in float64
    @staticmethod
    def curve(gains_ev, sigma: float = 2 ** 0.5) -> np.ndarray:
        """The nine weights w_k of the Gaussians at CENTRES for which the correction passes through gains_ev at the centres."""
        g = np.asarray(gains_ev, dtype=np.float64).reshape(-1)
        if g.shape != (9,):
            raise ValueError(f'gains_ev must have 9 values (the bands at -8 .. 0 EV), got {g.size}')
        if not np.all(np.isfinite(g)):
            raise ValueError(f'gains_ev must be finite, got {g.tolist()}')
        c = np.asarray(CENTRES)
        return np.linalg.solve(np.exp(-(c[:, None] - c[None, :]) ** 2 / (2.0 * float(sigma) ** 2)), g)

    @staticmethod
    def correction(ev, weights, sigma: float = 2 ** 0.5) -> np.ndarray:
        """corr(ev) = sum_k w_k exp(-(clip(ev, -8, 0) - c_k)^2 / (2 sigma^2)), in EV."""
        ev = np.clip(np.asarray(ev, dtype=np.float64), CENTRES[0], CENTRES[-1])
        c = np.asarray(CENTRES)
        return (np.asarray(weights, dtype=np.float64) * np.exp(-(ev[..., None] - c) ** 2 / (2.0 * float(sigma) ** 2))).sum(-1)

    @staticmethod
    def table_nodes() -> np.ndarray:
        """The mask values the table's entries stand at: 32 per octave, linear inside an octave, 2^-16 .. 2^4."""
        j = np.arange(TDK_TONEEQ_TABLE)
        return (1.0 + (j % TDK_TONEEQ_STEPS) / TDK_TONEEQ_STEPS) * 2.0 ** (TDK_TONEEQ_EV_MIN + j // TDK_TONEEQ_STEPS)

    @staticmethod
    def make_table(gains_ev, mask_exposure: float = 0.0, sigma: float = 2 ** 0.5) -> np.ndarray:
        """T[j] = float32(2 ** corr(log2(node j) + mask_exposure)): all-zero gains give exact ones."""
        w = ToneEqualizer.curve(gains_ev, sigma)
        return np.exp2(ToneEqualizer.correction(np.log2(ToneEqualizer.table_nodes()) + float(mask_exposure), w, sigma)).astype(np.float32)

    def _check_gains(self, gains_ev, mask_exposure) -> tuple[tuple[float, ...], float]:
        if isinstance(gains_ev, torch.Tensor):
            gains_ev = gains_ev.tolist()
        gains = tuple(float(v) for v in gains_ev)
        w = self.curve(gains, self.sigma)   # (refuses a wrong count and non-finite values)
        mask_exposure = float(mask_exposure)
        if not math.isfinite(mask_exposure):
            raise ValueError(f'mask_exposure must be finite, got {mask_exposure}')
        # the pole check: a curve that swings far outside its nodes between them (darktable: "the curve is ill-conditioned")
        between = self.correction(np.linspace(CENTRES[0], CENTRES[-1], 16 * 8 + 1), w, self.sigma)
        if between.max() > max(gains) + MAX_OVERSHOOT_EV or between.min() < min(gains) - MAX_OVERSHOOT_EV:
            raise ValueError(f'gains_ev give an ill-conditioned curve: between the bands it spans {between.min():.2f} .. {between.max():.2f} EV, '
                             f'the gains {min(gains):g} .. {max(gains):g} EV (more than {MAX_OVERSHOOT_EV:g} EV outside); smooth the gains or raise sigma')
        return gains, mask_exposure

    def set_gains(self, gains_ev, mask_exposure: float | None = None) -> None:
        """A new table in the SAME device tensor, copied in stream order from the host buffer the object keeps: calls enqueued
        afterwards on this stream, replays of a captured `process` among them, use it."""
        gains, exposure = self._check_gains(gains_ev, self.mask_exposure if mask_exposure is None else mask_exposure)
        self._gains_ev, self.mask_exposure = gains, exposure
        self._host_table.copy_(torch.from_numpy(self.make_table(gains, exposure, self.sigma)))
        if self._table is not None:
            self._table.copy_(self._host_table, non_blocking=True)

    @property
    def table(self) -> torch.Tensor | None:
        """The (641,) float32 gain table on the device (None where no GPU exists)."""
        return self._table

    @property
    def gains_ev(self) -> tuple[float, ...]:
        return self._gains_ev

    def __repr__(self):
        return (f'ToneEqualizer({self.width}x{self.height}, gains_ev={self._gains_ev}, cell={self.cell}, radius={self.radius}, eps={self.eps:g}, '
                f'mask_exposure={self.mask_exposure:g})')

    def workspace_bytes(self) -> int:
        return int(lib.tdk_toneeq_workspace_bytes(self.width, self.height, self.cell))

    def lds_bytes(self, dtype: torch.dtype = torch.float32) -> int:
        """The largest LDS use of a workgroup over the launches of a call on frames of this type (0: not a legal call)."""
        return int(lib.tdk_toneeq_lds_bytes(TAGS.get(dtype, -1), self.cell, self.radius))

    def _run(self, image: torch.Tensor, want_frame: bool, want_mask: bool):
        height, width, _, tag = self._float_frame(image, 'ToneEqualizer', 'image channels must be 3')
        if self._table is None or self._table.device != image.device:
            raise RuntimeError(f'ToneEqualizer was built for {None if self._table is None else self._table.device}, the image is on {image.device}')
        with torch.cuda.device(image.device):
            out = torch.empty_like(image) if want_frame else None
            mask = torch.empty((height, width), dtype=torch.float32, device=image.device) if want_mask else None
            rc = lib.tdk_toneeq(_ptr(image), _ptr(out), _ptr(mask), _ptr(self._workspace(image.device)), _ptr(self._table), width, height, tag, self.cell,
                                self.radius, self.eps, self._c_weights, 0, _stream())
        check(rc)
        return out, mask

    def process(self, image: torch.Tensor, return_mask: bool = False):
        """(H, W, 3) float32 or float16 -> the frame of the same type with every pixel scaled by its region's gain, not clamped.
        return_mask: (frame, mask) with the (H, W) float32 mask m the gains were looked up at."""
        out, mask = self._run(image, True, bool(return_mask))
        return (out, mask) if return_mask else out

    def mask(self, image: torch.Tensor) -> torch.Tensor:
        """The (H, W) float32 mask alone: no frame is written."""
        return self._run(image, False, True)[1]


__all__ = ['ToneEqualizer']
