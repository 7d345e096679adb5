"""Colour management (include/tdk_hip_lut.h: tdk_color_lut) -- a 3x3 matrix, shaper curves and a 3D look-up table, applied to every
pixel of an (..., 3) frame in this order by one kernel launch.  Every stage is optional.

    matrix    r' = (m0*r + m1*g) + m2*b, ...: a camera matrix, a white point adaptation, a channel mixer
    shaper    a 1D curve, one table for all channels or one per channel, sampled evenly over `shaper_domain` and interpolated
              linearly; input outside the domain takes the first or last entry
    lut       an (N, N, N, 3) table indexed [b, g, r] (red runs fastest: the memory order of a .cube file), sampled evenly over
              `lut_domain`, interpolated tetrahedrally (what grading tools do: the grey axis stays neutral) or trilinearly

Source and destination storage are independent: float32, float16 or uint8 each (uint8 codes stand for code / 255).  The exact float32
formulas are in the header; a NumPy restatement (tests/colorlut_spec.py) predicts the bits.  One launch on PyTorch's current stream,
no workspace, no synchronisation, no copy: capturable in a HIP graph from the first call, and bit-reproducible.  The tables are
checked on the host and uploaded once, when the object is built.

    look = ColorLUT.from_cube('film.cube', device)                   # a .cube file, 3D or 1D
    graded = look.process(tone_mapped_uint8)                         # uint8 in, uint8 out
    cam = ColorLUT.from_matrix(device, camera_to_working)            # the input colour transform
    linear = cam.process(demosaiced_half)                            # float16 in, float16 out
    display = ColorLUT(device, matrix=m, shaper=gamma_table, lut=gamut_lut).process(linear, out_dtype=torch.uint8)
"""

from __future__ import annotations

import ctypes
import math
import os

import torch

from ._frames import TAGS, require_cuda_device
from ._native import TDK_LUT_GLOBAL, TDK_LUT_MAX_SHAPER, TDK_LUT_MAX_SIZE, TDK_LUT_TETRAHEDRAL, TDK_LUT_TRILINEAR, check, lib
from ._stage import as_float32 as _f32
from .torch_darktable_extension import _ptr, _require, _stream

_INTERPOLATIONS = {'tetrahedral': TDK_LUT_TETRAHEDRAL, 'trilinear': TDK_LUT_TRILINEAR}


def _scale(entries: int, lo: float, hi: float, what: str) -> float:
    """float32(entries - 1) / (float32(hi) - float32(lo)), every operation in float32."""
    lo32, hi32 = torch.tensor(float(lo), dtype=torch.float32), torch.tensor(float(hi), dtype=torch.float32)
    scale = float(torch.tensor(float(entries - 1), dtype=torch.float32) / (hi32 - lo32))
    if not (math.isfinite(float(lo32)) and math.isfinite(float(hi32)) and math.isfinite(scale)):
        raise ValueError(f'{what} must be finite with distinct ends, got ({lo}, {hi})')
    return scale


def _host_table(values, what: str) -> torch.Tensor:
    table = torch.as_tensor(values).detach().to(device='cpu', dtype=torch.float32).contiguous()
    if not bool(torch.isfinite(table).all()):
        raise ValueError(f'{what} must be finite')
    return table


class ColorLUT:
    """A pointwise colour transform on (..., 3) frames; see the module's head for the stages.  `global_nodes = True` makes the kernel
    gather the nodes of a small LUT from global memory instead of LDS (tests and measurement: the bits are the same)."""

    GROUP = 16  # pixels a lane takes per step (csrc/colorlut.hip: CL_PIX)

    def __init__(self, device: torch.device, matrix=None, shaper=None, shaper_domain: tuple[float, float] = (0.0, 1.0), lut=None,
                 lut_domain=((0, 0, 0), (1, 1, 1)), interpolation: str = 'tetrahedral'):
        require_cuda_device(device)
        if interpolation not in _INTERPOLATIONS:
            raise ValueError(f"interpolation must be 'tetrahedral' or 'trilinear', got {interpolation!r}")
        self._device = device
        self.interpolation = interpolation
        self.global_nodes = False

        self.matrix: tuple[float, ...] | None = None
        if matrix is not None:
            m = torch.as_tensor(matrix).detach().to(device='cpu', dtype=torch.float32)
            if m.numel() != 9 or m.dim() > 2 or (m.dim() == 2 and tuple(m.shape) != (3, 3)):
                raise ValueError(f'matrix must be 3x3 (or 9 values, row-major), got shape {tuple(m.shape)}')
            self.matrix = tuple(float(v) for v in m.reshape(-1).tolist())
            if not all(math.isfinite(v) for v in self.matrix):
                raise ValueError(f'matrix must be finite, got {self.matrix}')
        self._c_matrix = (ctypes.c_float * 9)(*self.matrix) if self.matrix is not None else None

        self.shaper: torch.Tensor | None = None     # the host copy: (S,) or (3, S) float32
        self.shaper_lo, self.shaper_scale = 0.0, 0.0
        if shaper is not None:
            table = _host_table(shaper, 'shaper')
            if not (table.dim() == 1 or (table.dim() == 2 and table.shape[0] == 3)) or not 2 <= table.shape[-1] <= TDK_LUT_MAX_SHAPER:
                raise ValueError(f'shaper must be (S,) or (3, S) with S in 2..{TDK_LUT_MAX_SHAPER}, got shape {tuple(table.shape)}')
            if len(tuple(shaper_domain)) != 2:
                raise ValueError(f'shaper_domain must be (lo, hi), got {shaper_domain}')
            self.shaper = table
            self.shaper_lo = _f32(shaper_domain[0])
            self.shaper_scale = _scale(table.shape[-1], shaper_domain[0], shaper_domain[1], 'shaper_domain')

        self.lut: torch.Tensor | None = None        # the host copy: (N, N, N, 3) float32, indexed [b, g, r]
        self.lut_lo, self.lut_scale = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
        if lut is not None:
            table = _host_table(lut, 'lut')
            n = table.shape[0] if table.dim() == 4 else 0
            if tuple(table.shape) != (n, n, n, 3) or not 2 <= n <= TDK_LUT_MAX_SIZE:
                raise ValueError(f'lut must be (N, N, N, 3) with N in 2..{TDK_LUT_MAX_SIZE}, got shape {tuple(table.shape)}')
            lo, hi = (tuple(lut_domain[0]), tuple(lut_domain[1])) if len(tuple(lut_domain)) == 2 else ((), ())
            if len(lo) != 3 or len(hi) != 3:
                raise ValueError(f'lut_domain must be ((lo_r, lo_g, lo_b), (hi_r, hi_g, hi_b)), got {lut_domain}')
            self.lut = table
            self.lut_lo = tuple(_f32(v) for v in lo)
            self.lut_scale = tuple(_scale(n, lo[c], hi[c], 'lut_domain') for c in range(3))
        self._c_lut_lo, self._c_lut_scale = (ctypes.c_float * 3)(*self.lut_lo), (ctypes.c_float * 3)(*self.lut_scale)

        self._tables: dict[torch.device, tuple[torch.Tensor | None, torch.Tensor | None]] = {}
        if torch.cuda.is_available():   # (an object can be built and queried without a GPU; nothing runs there)
            self._upload(torch.device('cuda', torch.cuda.current_device()) if device.index is None else device)

    # ---- other ways to build one
    @staticmethod
    def from_matrix(device: torch.device, matrix) -> 'ColorLUT':
        """The matrix alone: an input colour transform."""
        return ColorLUT(device, matrix=matrix)

    @staticmethod
    def identity(device: torch.device, size: int) -> 'ColorLUT':
        """A 3D LUT of `size` nodes per axis over [0, 1] whose node (r, g, b) holds (r, g, b) / (size - 1)."""
        if int(size) != size or not 2 <= int(size) <= TDK_LUT_MAX_SIZE:
            raise ValueError(f'size must be an integer in 2..{TDK_LUT_MAX_SIZE}, got {size}')
        n = int(size)
        axis = torch.arange(n, dtype=torch.float32) / torch.tensor(float(n - 1), dtype=torch.float32)
        b, g, r = torch.meshgrid(axis, axis, axis, indexing='ij')
        return ColorLUT(device, lut=torch.stack((r, g, b), dim=-1))

    @staticmethod
    def from_cube(path_or_text, device: torch.device, **kw) -> 'ColorLUT':
        """A .cube file (Adobe / Resolve text format): a path, or the text itself (a string with a line break).  A 3D file becomes
        the LUT with its DOMAIN_MIN / DOMAIN_MAX (or Resolve's LUT_3D_INPUT_RANGE / LUT_1D_INPUT_RANGE lo hi); a 1D file becomes a
        three-table shaper (its domain must be the same for the three channels).  Further keywords (matrix, interpolation, ...) go to the constructor.  Malformed input raises ValueError naming
        the line."""
        if isinstance(path_or_text, os.PathLike) or (isinstance(path_or_text, str) and '\n' not in path_or_text):
            with open(path_or_text, 'r', encoding='utf-8', errors='replace') as f:
                text = f.read()
        else:
            text = str(path_or_text)
        kind, size, lo, hi, rows = parse_cube(text)
        if kind == '3D':
            return ColorLUT(device, lut=torch.tensor(rows, dtype=torch.float32).reshape(size, size, size, 3), lut_domain=(lo, hi), **kw)
        if len(set(lo)) != 1 or len(set(hi)) != 1:
            raise ValueError(f'a 1D .cube file needs the same domain for the three channels, got DOMAIN_MIN {lo} DOMAIN_MAX {hi}')
        return ColorLUT(device, shaper=torch.tensor(rows, dtype=torch.float32).t().contiguous(), shaper_domain=(lo[0], hi[0]), **kw)

    # ---- queries
    @property
    def shaper_size(self) -> int:
        return 0 if self.shaper is None else int(self.shaper.shape[-1])

    @property
    def shaper_tables(self) -> int:
        return 3 if self.shaper is not None and self.shaper.dim() == 2 else 1

    @property
    def lut_size(self) -> int:
        return 0 if self.lut is None else int(self.lut.shape[0])

    def _flags(self) -> int:
        return TDK_LUT_GLOBAL if self.global_nodes else 0

    def lds_bytes(self) -> int:
        """LDS one workgroup takes: the shaper tables and, when the LUT is staged there, its nodes."""
        return int(lib.tdk_lut_lds_bytes(self.shaper_size, self.shaper_tables, self.lut_size, self._flags()))

    def __repr__(self):
        parts = []
        if self.matrix is not None:
            parts.append('matrix')
        if self.shaper is not None:
            parts.append(f'shaper={self.shaper_tables}x{self.shaper_size}')
        if self.lut is not None:
            parts.append(f'lut={self.lut_size}^3 {self.interpolation}')
        return f"ColorLUT({', '.join(parts) if parts else 'no stage'}, lds={self.lds_bytes()})"

    # ---- the call
    def _upload(self, device: torch.device) -> tuple[torch.Tensor | None, torch.Tensor | None]:
        tables = self._tables.get(device)
        if tables is None:
            tables = self._tables[device] = tuple(None if t is None else t.to(device).contiguous() for t in (self.shaper, self.lut))
        return tables

    def process(self, frame: torch.Tensor, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """(..., 3) float32, float16 or uint8 -> the same shape in `out_dtype` (None: the input's type)."""
        if frame.dim() < 1 or frame.shape[-1] != 3:
            raise ValueError(f'frame must have three channels in its last dimension, got shape {tuple(frame.shape)}')
        _require(frame.dtype in TAGS, 'Input tensor must be float32, float16 or uint8')
        out_dtype = frame.dtype if out_dtype is None else out_dtype
        if out_dtype not in TAGS:
            raise ValueError(f'out_dtype must be float32, float16 or uint8, got {out_dtype}')
        _require(frame.is_cuda, 'Input must be on CUDA device')
        _require(frame.is_contiguous(), 'Input must be contiguous')
        shaper, lut = self._upload(frame.device)
        with torch.cuda.device(frame.device):
            out = torch.empty(frame.shape, dtype=out_dtype, device=frame.device)
            if frame.numel() == 0:
                return out
            rc = lib.tdk_color_lut(_ptr(frame), TAGS[frame.dtype], _ptr(out), TAGS[out_dtype], frame.numel() // 3, self._c_matrix, _ptr(shaper),
                                   self.shaper_size, self.shaper_tables, self.shaper_lo, self.shaper_scale, _ptr(lut), self.lut_size,
                                   self._c_lut_lo, self._c_lut_scale, _INTERPOLATIONS[self.interpolation], self._flags(), _stream())
        check(rc)
        return out


def parse_cube(text: str):
    """('3D' | '1D', size, DOMAIN_MIN, DOMAIN_MAX, rows) of the text of a .cube file; rows is a list of [r, g, b]."""
    kind, size, size_line = None, 0, 0
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    rows: list[list[float]] = []
    number = 0
    for number, raw in enumerate(text.splitlines(), start=1):
        line = raw.strip()
        if not line or line.startswith('#'):
            continue
        where = f'line {number}: {line!r}'
        words = line.split()
        key = words[0].upper()
        if key == 'TITLE':
            continue
        if key in ('LUT_3D_SIZE', 'LUT_1D_SIZE'):
            if kind is not None:
                raise ValueError(f'{where}: a second size (line {size_line} has one); files with a 1D and a 3D table are not supported')
            if len(words) != 2 or not words[1].isdigit():
                raise ValueError(f'{where}: expected one integer')
            kind, size, size_line = key[4:6], int(words[1]), number
            limit = TDK_LUT_MAX_SIZE if kind == '3D' else TDK_LUT_MAX_SHAPER
            if not 2 <= size <= limit:
                raise ValueError(f'{where}: size must be 2..{limit}')
            continue
        if key in ('DOMAIN_MIN', 'DOMAIN_MAX', 'LUT_1D_INPUT_RANGE', 'LUT_3D_INPUT_RANGE'):
            want = 3 if key.startswith('DOMAIN') else 2
            try:
                values = tuple(float(w) for w in words[1:])
            except ValueError:
                values = ()
            if len(values) != want or not all(math.isfinite(v) for v in values):
                raise ValueError(f'{where}: expected {want} finite numbers')
            if key == 'DOMAIN_MIN':
                lo = values
            elif key == 'DOMAIN_MAX':
                hi = values
            else:
                lo, hi = (values[0],) * 3, (values[1],) * 3
            continue
        try:
            values = [float(w) for w in words]
        except ValueError:
            raise ValueError(f'{where}: not a keyword of the format and not a row of numbers') from None
        if len(values) != 3:
            raise ValueError(f'{where}: a row has three numbers, got {len(values)}')
        if not all(math.isfinite(v) for v in values):
            raise ValueError(f'{where}: non-finite value')
        if kind is None:
            raise ValueError(f'{where}: a row in front of LUT_3D_SIZE / LUT_1D_SIZE')
        rows.append(values)
        if len(rows) > (size ** 3 if kind == '3D' else size):
            raise ValueError(f'{where}: more rows than the {size ** 3 if kind == "3D" else size} that line {size_line} announces')
    if kind is None:
        raise ValueError(f'line {number}: end of text without LUT_3D_SIZE or LUT_1D_SIZE')
    expected = size ** 3 if kind == '3D' else size
    if len(rows) != expected:
        raise ValueError(f'line {number}: end of text after {len(rows)} rows, line {size_line} announces {expected}')
    return kind, size, lo, hi, rows


__all__ = ['ColorLUT']
