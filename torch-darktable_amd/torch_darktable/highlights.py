"""White balance that reconstructs clipped highlights (include/tdk_hip_highlights.h: tdk_highlights) -- the stage darktable calls
highlight reconstruction, on the white-balanced mosaic in front of the demosaic.  In a chain it takes the place of
`apply_white_balance`.

    v = L * gain[colour]                          L: the linear mosaic BEFORE white balance, 1.0 = white level
    a site with L >= threshold is clipped: the sensor has lost its value
    'clip'     every site is cut at the lowest clipping level of the three colours: min(threshold * gain) -- neutral, flat highlights
    'opposed'  a clipped site becomes max(v, ref + chroma[colour]): ref is the mean of the two OTHER colours over its 3x3
               neighbourhood, chroma a per-frame colour offset measured on the unclipped sites next to clipped ones
               (darktable's "inpaint opposed", with the means taken in the linear domain)

The result is not clamped from above.  The exact float32 formulas are in the header; a NumPy restatement
(tests/test_highlights_spec.py) predicts the bits.  At most two launches on PyTorch's current stream, no synchronisation, no
atomics; the few KB of workspace belong to the object, one per stream: capturable in a HIP graph from the first call, and
bit-reproducible.

    h = Highlights(device, (4096, 3072), BayerPattern.RGGB)
    mosaic = h.process(decode12_float(raw_bytes, ...).view(3072, 4096), gains)       # (H, W) float32, white-balanced
    rgb = RCD(device, (4096, 3072), BayerPattern.RGGB).process(mosaic.unsqueeze(-1))

A caller who tracks `chrominance` across frames (as the processor averages its bounds) can feed it back with
`process(..., chrominance=c)`: that skips the statistics launch.
"""

from __future__ import annotations

import math

import torch

from ._mosaic import FLOAT_TAGS, MosaicStage, check_pattern, out_dtype_of
from ._native import TDK_HL_CLIP, TDK_HL_OPPOSED, check, lib
from .bayer import BayerPattern
from .torch_darktable_extension import _pattern, _ptr, _stream

MAX_GAIN = 64.0
_MODES = {'clip': TDK_HL_CLIP, 'opposed': TDK_HL_OPPOSED}


class Highlights(MosaicStage):
    """White-balance (H, W) mosaics of one size and reconstruct their clipped sites; image_size is (width, height), both even."""

    TILE = (128, 16)  # (width, height) of one workgroup's tile (csrc/highlights.hip: HL_TW, HL_TH)

    def __init__(self, device: torch.device, image_size: tuple[int, int], bayer_pattern: BayerPattern, mode: str = 'opposed',
                 threshold: float = 0.98, low: float = 0.2, min_count: int = 64):
        super().__init__(device, image_size)
        self._check_even('Image')
        check_pattern(bayer_pattern)
        if mode not in _MODES:
            raise ValueError(f"mode must be 'opposed' or 'clip', got {mode!r}")
        if not 0.0 < float(threshold) <= 1.0:
            raise ValueError(f'threshold must lie in (0, 1], got {threshold}')
        if not 0.0 <= float(low) < 1.0:
            raise ValueError(f'low must lie in [0, 1), got {low}')
        if int(min_count) != min_count or not 1 <= int(min_count) < 2 ** 31:
            raise ValueError(f'min_count must be an integer >= 1, got {min_count}')
        self.bayer_pattern, self.mode = bayer_pattern, mode
        self.threshold, self.low, self.min_count = float(threshold), float(low), int(min_count)
        self._keep_workspace()

    def __repr__(self):
        return (f'Highlights({self.width}x{self.height}, {self.bayer_pattern.name}, mode={self.mode}, threshold={self.threshold:g}, '
                f'low={self.low:g}, min_count={self.min_count})')

    def lds_bytes(self) -> int:
        """The largest LDS use of a workgroup over the launches of a call (0: the streaming 'clip' mode)."""
        return int(lib.tdk_highlights_lds_bytes(_MODES[self.mode]))

    @staticmethod
    def workspace_bytes() -> int:
        return int(lib.tdk_highlights_workspace_bytes())

    def _tag(self, mosaic: torch.Tensor) -> int:
        assert mosaic.dim() == 2, f'mosaic must have 2 dimensions, got {mosaic.shape}'
        self._check_mosaic(mosaic)
        return FLOAT_TAGS[mosaic.dtype]

    @staticmethod
    def _three(values, what: str, device: torch.device, limit: float | None) -> torch.Tensor:
        """Three float32 values on `device`.  Host values are checked; a tensor already on a device is taken as it is (looking at it
        would synchronise)."""
        t = torch.as_tensor(values)
        if t.numel() != 3:
            raise ValueError(f'{what} must have 3 elements (R, G, B), got {t.numel()}')
        if not t.is_cuda:
            host = [float(v) for v in t.reshape(-1).tolist()]
            if not all(math.isfinite(v) for v in host):
                raise ValueError(f'{what} must be finite, got {host}')
            if limit is not None and not all(0.0 < v <= limit for v in host):
                raise ValueError(f'{what} must lie in (0, {limit:g}], got {host}')
        return t.reshape(-1).to(device=device, dtype=torch.float32).contiguous()

    def process(self, mosaic: torch.Tensor, white_balance, out_dtype: torch.dtype = torch.float32, chrominance=None) -> torch.Tensor:
        """(height, width) float32 or float16 linear mosaic before white balance -> the white-balanced mosaic of `out_dtype`, clipped
        sites reconstructed, not clamped from above.  white_balance: 3 gains (R, G, B) in (0, 64]; a float32 tensor on the device keeps
        the call free of copies.  chrominance ('opposed' only): three values, say from `chrominance()`, used as they are -- the
        statistics launch is skipped."""
        tag = self._tag(mosaic)
        out_dtype_of(out_dtype, None)
        if chrominance is not None and self.mode != 'opposed':
            raise ValueError(f"chrominance is for mode 'opposed', the object has mode {self.mode!r}")
        gains = self._three(white_balance, 'white_balance', mosaic.device, MAX_GAIN)
        chroma = self._three(chrominance, 'chrominance', mosaic.device, None) if chrominance is not None else None
        with torch.cuda.device(mosaic.device):
            out = torch.empty((self.height, self.width), dtype=out_dtype, device=mosaic.device)
            workspace = self._workspace(mosaic.device) if self.mode == 'opposed' and chroma is None else None
            rc = lib.tdk_highlights(_ptr(mosaic), tag, _ptr(out), FLOAT_TAGS[out_dtype], _ptr(workspace), self.width, self.height, _pattern(self.bayer_pattern),
                                    _ptr(gains), self.threshold, self.low, self.min_count, _MODES[self.mode], _ptr(chroma), _stream())
        check(rc)
        return out

    def _gather(self, mosaic: torch.Tensor, white_balance, stats: torch.Tensor | None, chroma: torch.Tensor | None) -> None:
        tag = self._tag(mosaic)
        gains = self._three(white_balance, 'white_balance', mosaic.device, MAX_GAIN)
        with torch.cuda.device(mosaic.device):
            rc = lib.tdk_highlights_chrominance(_ptr(mosaic), tag, _ptr(self._workspace(mosaic.device)), self.width, self.height, _pattern(self.bayer_pattern),
                                                _ptr(gains), self.threshold, self.low, self.min_count, _ptr(stats), _ptr(chroma), _stream())
        check(rc)

    def chrominance(self, mosaic: torch.Tensor, white_balance) -> torch.Tensor:
        """The per-frame colour offset of mode 'opposed': a (3,) float32 device tensor (R, G, B); 0 for a colour with fewer than
        min_count contributing sites."""
        self._tag(mosaic)
        chroma = torch.empty(3, dtype=torch.float32, device=mosaic.device)
        self._gather(mosaic, white_balance, None, chroma)
        return chroma

    def statistics(self, mosaic: torch.Tensor, white_balance) -> tuple[torch.Tensor, torch.Tensor]:
        """(sum, cnt), each a (3,) int64 device tensor: the sums of rint(d * 2**20) and the counts of the contributing sites per colour."""
        self._tag(mosaic)
        stats = torch.empty(6, dtype=torch.int64, device=mosaic.device)
        self._gather(mosaic, white_balance, stats, None)
        return stats[:3], stats[3:]


__all__ = ['Highlights']
