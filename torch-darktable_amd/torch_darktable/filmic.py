"""Scene-referred tone mapping (include/tdk_hip_filmic.h: tdk_filmic) -- the display transform of darktable's scene-referred
workflow, "filmic rgb" and "sigmoid": a tone curve over log2 of a pixel NORM, applied to the channel ratios.

The three mappers behind `tonemap` are per-channel curves steered by image metrics.  This stage has an explicit black and white
exposure, keeps a pixel's chromaticity through the curve, and lets saturation go towards white so that highlights clip achromatically:

    p        = max(x * exposure, 0)                          per channel; `exposure` is one float in device memory
    N        = max(p) | luminance(p) | sum p^3 / sum p^2     the norm ('none': every channel on its own, no ratios)
    y, d     = T(log2 N), D(log2 N)                          two tables, 32 nodes per octave over 2^-20 .. 2^12: the curve's
                                                             display-linear value and the saturation it keeps there
    o_c      = y * (1 + d * (p_c / N - 1))                   the ratios, pulled towards grey by 1 - d
    o        -> pulled towards (y, y, y) until max(o) <= 1   the gamut step; only 'luma' and 'power' need it
    v_c      = G(o_c)                                        the display encoding, a third table over 2^-16 .. 1 (sRGB, a gamma, or none)

The exact float32 formulas of the device are in the header, and a NumPy restatement (tests/filmic_spec.py) predicts the bits.  The
host builds the tables in float64 and rounds once.  One launch on PyTorch's current stream, no workspace, no synchronisation:
capturable in a HIP graph from the first call, and bit-reproducible.  Exposure and tables are read from device memory by every call,
so a captured call follows `set_exposure` and `set_curve`.

    f = Filmic(device)                                       # grey 0.18, black 8 EV below, white where the curve reaches 1
    display = f.process(linear)                              # (..., 3) float32 or float16 -> uint8, sRGB
    f.set_exposure(0.18 / stats.percentiles(...)[...])       # a device tensor: nothing waits for it
    s = Filmic.sigmoid(device, contrast=1.6)                 # darktable's sigmoid
    c = Filmic.from_curve(device, lambda x: x / (1 + x))     # any curve of one's own
"""

from __future__ import annotations

import math

import torch

from ._frames import TAGS, require_cuda_device
from ._native import (TDK_F16, TDK_F32, TDK_FILMIC_ENC_EV_MIN, TDK_FILMIC_ENC_TABLE, TDK_FILMIC_EV_MIN, TDK_FILMIC_LUMA, TDK_FILMIC_MAX, TDK_FILMIC_NONE,
                      TDK_FILMIC_POWER, TDK_FILMIC_STEPS, TDK_FILMIC_TABLE, check, lib)
from ._stage import as_float32, home_device, luma_weights
from .torch_darktable_extension import _ptr, _require, _stream

NORMS = {'max': TDK_FILMIC_MAX, 'luma': TDK_FILMIC_LUMA, 'power': TDK_FILMIC_POWER, 'none': TDK_FILMIC_NONE}
_SPLINE = ('grey', 'black_ev', 'white_ev', 'contrast', 'latitude', 'target', 'output_power', 'desaturate')


def _nodes(ev_min: int, entries: int) -> torch.Tensor:
    """The float64 positions of the nodes of a table: (1 + (j % 32) / 32) * 2^(j / 32 + ev_min)."""
    j = torch.arange(entries, dtype=torch.int64)
    return (1.0 + (j % TDK_FILMIC_STEPS).to(torch.float64) / TDK_FILMIC_STEPS) * torch.pow(torch.tensor(2.0, dtype=torch.float64), (j // TDK_FILMIC_STEPS + ev_min).to(torch.float64))


def _smooth(u: torch.Tensor) -> torch.Tensor:
    u = u.clamp(0.0, 1.0)
    return u * u * (3.0 - 2.0 * u)


def _hermite(t, x0, x1, v0, v1, m0, m1):
    """The cubic through (x0, v0) and (x1, v1) with the slopes m0 and m1 there."""
    h = x1 - x0
    s = (t - x0) / h
    s2, s3 = s * s, s * s * s
    return (2 * s3 - 3 * s2 + 1) * v0 + (s3 - 2 * s2 + s) * h * m0 + (-2 * s3 + 3 * s2) * v1 + (s3 - s2) * h * m1


def _finite(value, what: str) -> float:
    value = float(value)
    if not math.isfinite(value):
        raise ValueError(f'{what} must be finite, got {value}')
    return value


def filmic_spline(grey=0.18, black_ev=-8.0, white_ev=None, contrast=1.5, latitude=0.25, target=(0.0, 0.1845, 1.0), output_power=None, desaturate=(0.0, 1.0)):
    """The checked parameters of the filmic curve as a dict, with what follows from them (t_g, t_lo, t_hi, v_b, v_g, v_w, v_lo, v_hi
    and the power p).  Raises ValueError for parameters outside their ranges and for those whose toe or shoulder would not be
    monotone (Fritsch and Carlson: a Hermite segment between a slope of 0 and a slope of `contrast` is monotone when
    contrast <= 3 * its secant)."""
    grey = _finite(grey, 'grey')
    if not grey > 0.0:
        raise ValueError(f'grey must be > 0, got {grey}')
    black_ev = _finite(black_ev, 'black_ev')
    white_ev = math.log2(1.0 / grey) if white_ev is None else _finite(white_ev, 'white_ev')
    if not (black_ev < 0.0 < white_ev):
        raise ValueError(f'black_ev must be < 0 and white_ev > 0 (exposures relative to grey), got {black_ev} and {white_ev}')
    contrast, latitude = _finite(contrast, 'contrast'), _finite(latitude, 'latitude')
    if not contrast > 0.0:
        raise ValueError(f'contrast must be > 0, got {contrast}')
    if not 0.0 <= latitude < 1.0:
        raise ValueError(f'latitude must be in [0, 1), got {latitude}')
    target = tuple(float(v) for v in target)
    if len(target) != 3 or not (0.0 <= target[0] < target[1] < target[2] <= 1.0):
        raise ValueError(f'target must be (black, grey, white) with 0 <= black < grey < white <= 1, got {target}')
    desaturate = tuple(float(v) for v in desaturate)
    if len(desaturate) != 2 or not all(0.0 <= v <= 1.0 for v in desaturate):
        raise ValueError(f'desaturate must be (shadows, highlights), each in 0..1, got {desaturate}')
    t_g = -black_ev / (white_ev - black_ev)
    p = math.log(target[1]) / math.log(t_g) if output_power is None else _finite(output_power, 'output_power')
    if not p > 0.0:
        raise ValueError(f'output_power must be > 0, got {p}')
    v_b, v_g, v_w = (v ** (1.0 / p) for v in target)
    t_lo, t_hi = t_g - latitude * t_g, t_g + latitude * (1.0 - t_g)
    v_lo, v_hi = v_g - contrast * (t_g - t_lo), v_g + contrast * (t_hi - t_g)
    if not (v_b < v_lo and v_hi < v_w):
        raise ValueError(f'contrast {contrast:g} over latitude {latitude:g} leaves the range of the curve: the linear part runs from {v_lo:.4g} to {v_hi:.4g}, '
                         f'black and white are at {v_b:.4g} and {v_w:.4g}')
    toe, shoulder = (v_lo - v_b) / t_lo, (v_w - v_hi) / (1.0 - t_hi)
    if contrast > 3.0 * toe or contrast > 3.0 * shoulder:
        raise ValueError(f'contrast {contrast:g} would make the curve swing: it must be <= 3 x the slope of the toe ({toe:.4g}) and of the shoulder ({shoulder:.4g}); '
                         'lower the contrast or the latitude, or widen black_ev / white_ev')
    return dict(grey=grey, black_ev=black_ev, white_ev=white_ev, contrast=contrast, latitude=latitude, target=target, output_power=p, desaturate=desaturate,
                t_g=t_g, t_lo=t_lo, t_hi=t_hi, v_b=v_b, v_g=v_g, v_w=v_w, v_lo=v_lo, v_hi=v_hi)


def filmic_curve(x: torch.Tensor, s: dict) -> tuple[torch.Tensor, torch.Tensor]:
    """(T, D) of the filmic curve `s` (what filmic_spline returns) at the float64 scene values x > 0."""
    t = ((torch.log2(x / s['grey']) - s['black_ev']) / (s['white_ev'] - s['black_ev'])).clamp(0.0, 1.0)
    c, t_g, t_lo, t_hi = s['contrast'], s['t_g'], s['t_lo'], s['t_hi']
    v = s['v_g'] + c * (t - t_g)
    v = torch.where(t < t_lo, _hermite(t, 0.0, t_lo, s['v_b'], s['v_lo'], 0.0, c), v)
    v = torch.where(t > t_hi, _hermite(t, t_hi, 1.0, s['v_hi'], s['v_w'], c, 0.0), v)
    lo, hi = s['desaturate']
    d = 1.0 - hi * _smooth((t - t_hi) / (1.0 - t_hi)) - lo * _smooth((t_lo - t) / t_lo)
    return v.clamp_min(0.0) ** s['output_power'], d.clamp(0.0, 1.0)


def sigmoid_curve(x: torch.Tensor, grey: float, contrast: float, target_grey: float, desaturate: float, desaturate_ev: tuple[float, float]):
    """(T, D) of darktable's sigmoid at the float64 scene values x > 0: a log-logistic curve through (grey, target_grey); saturation
    goes between the two exposures of desaturate_ev (relative to grey)."""
    y = 1.0 / (1.0 + (grey / x) ** contrast * (1.0 / target_grey - 1.0))
    ev = torch.log2(x / grey)
    d = 1.0 - desaturate * _smooth((ev - desaturate_ev[0]) / (desaturate_ev[1] - desaturate_ev[0]))
    return y, d


def encoding_curve(encoding: str | None):
    """The float64 function of an encoding's name: 'srgb', 'gamma:<g>' (v = o^(1/g)); None for None."""
    if encoding is None:
        return None
    if encoding == 'srgb':
        return lambda o: torch.where(o <= 0.0031308, 12.92 * o, 1.055 * o.clamp_min(0.0031308) ** (1.0 / 2.4) - 0.055)
    if isinstance(encoding, str) and encoding.startswith('gamma:'):
        try:
            g = float(encoding[6:])
        except ValueError:
            g = float('nan')
        if math.isfinite(g) and g > 0.0:
            return lambda o: o ** (1.0 / g)
    raise ValueError(f"encoding must be 'srgb', 'gamma:<g>' with g > 0, or None, got {encoding!r}")


def _table(values, entries: int, what: str) -> torch.Tensor:
    table = torch.as_tensor(values).detach().to(device='cpu', dtype=torch.float64).reshape(-1)
    if table.numel() != entries:
        raise ValueError(f'{what} must give {entries} values, one per node, got {table.numel()}')
    table = table.to(torch.float32)   # rounded once
    if not bool(torch.isfinite(table).all()):
        raise ValueError(f'{what} must be finite as float32')
    return table


class Filmic:
    """A tone curve on (..., 3) scene-linear frames; see the module's head.  The constructor builds darktable's filmic spline:
    t = (log2(x / grey) - black_ev) / (white_ev - black_ev) clamped to 0..1 runs through a straight part of slope `contrast` around
    grey, `latitude` of the way to either end, and cubic Hermite segments that end flat at (0, black) and (1, white); the result is
    raised to `output_power` (None: the power that puts grey on the diagonal, v(t_g) = t_g).  white_ev None: log2(1 / grey), so that a
    scene value of 1 is display white.  target: the display-linear values of black, grey and white.  desaturate: how much saturation
    goes towards black and towards white (0..1 each).  norm: 'max', 'luma' (weights), 'power' or 'none'.  Parameters whose curve
    would not be monotone raise ValueError."""

    GROUP = 16  # pixels a lane takes per step (csrc/filmic.hip: FM_PIX)

    def __init__(self, device: torch.device, grey: float = 0.18, black_ev: float = -8.0, white_ev: float | None = None, contrast: float = 1.5, latitude: float = 0.25,
                 target: tuple[float, float, float] = (0.0, 0.1845, 1.0), output_power: float | None = None, desaturate: tuple[float, float] = (0.0, 1.0),
                 norm: str = 'max', encoding: str | None = 'srgb', weights=None):
        spline = filmic_spline(grey, black_ev, white_ev, contrast, latitude, target, output_power, desaturate)
        self._setup(device, norm, encoding, weights)
        self._spline: dict | None = dict(spline, white_ev=white_ev, output_power=output_power)   # as asked for: None stays None under set_curve
        self.parameters = spline
        self._install(*self._tables(lambda x: filmic_curve(x, spline)))

    @staticmethod
    def sigmoid(device: torch.device, grey: float = 0.18, contrast: float = 1.5, target_grey: float = 0.1845, desaturate: float = 1.0,
                desaturate_ev: tuple[float, float] = (0.0, 6.0), norm: str = 'max', encoding: str | None = 'srgb', weights=None) -> 'Filmic':
        """darktable's sigmoid: y = 1 / (1 + (grey / x)^contrast * (1 / target_grey - 1)), which needs no black or white exposure;
        `desaturate` of the saturation goes between the exposures desaturate_ev (relative to grey)."""
        grey, contrast, target_grey, desaturate = _finite(grey, 'grey'), _finite(contrast, 'contrast'), _finite(target_grey, 'target_grey'), _finite(desaturate, 'desaturate')
        if not (grey > 0.0 and contrast > 0.0):
            raise ValueError(f'grey and contrast must be > 0, got {grey} and {contrast}')
        if not 0.0 < target_grey < 1.0:
            raise ValueError(f'target_grey must be in (0, 1), got {target_grey}')
        ev = tuple(float(v) for v in desaturate_ev)
        if not 0.0 <= desaturate <= 1.0 or len(ev) != 2 or not (math.isfinite(ev[0]) and math.isfinite(ev[1]) and ev[0] < ev[1]):
            raise ValueError(f'desaturate must be in 0..1 and desaturate_ev two rising exposures, got {desaturate} and {desaturate_ev}')
        self = Filmic.__new__(Filmic)
        self._setup(device, norm, encoding, weights)
        self._spline = None
        self.parameters = dict(grey=grey, contrast=contrast, target_grey=target_grey, desaturate=desaturate, desaturate_ev=ev)
        self._install(*self._tables(lambda x: sigmoid_curve(x, grey, contrast, target_grey, desaturate, ev)))
        return self

    @staticmethod
    def from_curve(device: torch.device, fn, desaturation=None, norm: str = 'max', encoding: str | None = 'srgb', weights=None) -> 'Filmic':
        """The tables of a caller's own functions: fn(x) is the display-linear value of the scene value x (exposure applied),
        desaturation(x) the saturation kept there (None: all of it).  Both take the float64 tensor of table_nodes() and return as
        many values."""
        self = Filmic.__new__(Filmic)
        self._setup(device, norm, encoding, weights)
        self._spline = None
        self.parameters = {}
        self._install(*self._tables(lambda x: (fn(x), torch.ones_like(x) if desaturation is None else desaturation(x))))
        return self

    @staticmethod
    def table_nodes() -> torch.Tensor:
        """The scene values at which the curve is sampled: TDK_FILMIC_TABLE float64 values from 2^-20 to 2^12, 32 per octave."""
        return _nodes(TDK_FILMIC_EV_MIN, TDK_FILMIC_TABLE)

    @staticmethod
    def encoding_nodes() -> torch.Tensor:
        """The display-linear values at which the encoding is sampled: TDK_FILMIC_ENC_TABLE float64 values from 2^-16 to 1."""
        return _nodes(TDK_FILMIC_ENC_EV_MIN, TDK_FILMIC_ENC_TABLE)

    # ---- construction
    def _setup(self, device: torch.device, norm: str, encoding: str | None, weights) -> None:
        require_cuda_device(device)
        if norm not in NORMS:
            raise ValueError(f'norm must be one of {tuple(NORMS)}, got {norm!r}')
        self.weights, self._c_weights = luma_weights(weights)
        oetf = encoding_curve(encoding)
        self._device = device
        self.norm, self.encoding = norm, encoding
        self.host_encode = None if oetf is None else _table(oetf(self.encoding_nodes()), TDK_FILMIC_ENC_TABLE, 'encoding')
        self.host_curve: torch.Tensor | None = None     # (2, TDK_FILMIC_TABLE) float32: T, D
        self._host_exposure = 1.0
        self._curve: torch.Tensor | None = None
        self._encode: torch.Tensor | None = None
        self._exposure: torch.Tensor | None = None
        if torch.cuda.is_available():   # (an object can be built and queried without a GPU; nothing runs there)
            where = home_device(device)
            self._curve = torch.zeros((2, TDK_FILMIC_TABLE), dtype=torch.float32, device=where)
            self._exposure = torch.ones(1, dtype=torch.float32, device=where)
            self._encode = None if self.host_encode is None else self.host_encode.to(where)

    def _tables(self, curve) -> tuple[torch.Tensor, torch.Tensor]:
        t, d = curve(self.table_nodes())
        t, d = _table(t, TDK_FILMIC_TABLE, 'the curve'), _table(d, TDK_FILMIC_TABLE, 'the desaturation')
        if not bool(((d >= 0.0) & (d <= 1.0)).all()):
            raise ValueError('the desaturation must stay in 0..1')
        return t, d

    def _install(self, t: torch.Tensor, d: torch.Tensor) -> None:
        self.host_curve = torch.stack((t, d)).contiguous()   # a new tensor per call: a copy in flight keeps reading the old one
        if self._curve is not None:
            self._curve.copy_(self.host_curve, non_blocking=True)

    # ---- queries
    @property
    def exposure(self) -> torch.Tensor | None:
        """The object's (1,) float32 device tensor: the factor every sample is multiplied by (None where no GPU exists)."""
        return self._exposure

    @property
    def curve_table(self) -> torch.Tensor | None:
        """The object's (2, TDK_FILMIC_TABLE) float32 device tensor: T, D (None where no GPU exists; host_curve is its host copy)."""
        return self._curve

    @property
    def encode_table(self) -> torch.Tensor | None:
        """The object's (TDK_FILMIC_ENC_TABLE,) float32 device tensor G; None without an encoding or a GPU (host_encode: the host copy)."""
        return self._encode

    @property
    def lds_bytes(self) -> int:
        """LDS one workgroup takes: the three tables."""
        return int(lib.tdk_filmic_lds_bytes())

    def __repr__(self):
        kind = 'filmic' if self._spline is not None else 'sigmoid' if self.parameters else 'curve'
        return f"Filmic({kind}, norm='{self.norm}', encoding={self.encoding!r}, lds={self.lds_bytes})"

    # ---- state that captured calls follow
    def set_exposure(self, value) -> None:
        """The factor in front of the curve, for the calls that follow: a number, or a float32 device tensor of one value, which is
        copied on the device.  Written in stream order, nothing waits: a value computed on the stream (FrameStats percentiles) feeds a
        captured `process`, whose replays read what is there."""
        if isinstance(value, torch.Tensor):
            if value.dtype != torch.float32 or value.numel() != 1:
                raise ValueError(f'exposure must be a number or a float32 tensor of one value, got {value.dtype} {tuple(value.shape)}')
            if self._exposure is not None:
                _require(value.device == self._exposure.device, f'exposure is on {value.device}, Filmic on {self._exposure.device}')
                self._exposure.copy_(value.reshape(1), non_blocking=True)
            return
        value = as_float32(_finite(value, 'exposure'))
        if not (math.isfinite(value) and value >= 0.0):
            raise ValueError(f'exposure must be finite and >= 0 as a float32, got {value}')
        self._host_exposure = value
        if self._exposure is not None:
            self._exposure.fill_(value)

    def set_curve(self, fn=None, desaturation=None, **parameters) -> None:
        """Rewrite T and D in the object's tensors, in stream order.  With fn (and desaturation): the tables of from_curve.  Without:
        the filmic spline with the object's parameters changed by the keywords (grey, black_ev, white_ev, contrast, latitude, target,
        output_power, desaturate); only an object built by the constructor has them.  A refused change leaves the object as it was."""
        if fn is not None:
            if parameters:
                raise ValueError(f'set_curve takes a function or spline parameters, not both: {sorted(parameters)}')
            tables = self._tables(lambda x: (fn(x), torch.ones_like(x) if desaturation is None else desaturation(x)))
            self._spline, self.parameters = None, {}
            self._install(*tables)
            return
        if self._spline is None:
            raise ValueError('this Filmic was not built from the spline: give set_curve a function')
        unknown = sorted(set(parameters) - set(_SPLINE))
        if unknown or desaturation is not None:
            raise ValueError(f'set_curve takes the spline parameters {_SPLINE}, got {unknown or "desaturation"}')
        asked = {k: parameters.get(k, self._spline[k]) for k in _SPLINE}
        spline = filmic_spline(**asked)
        tables = self._tables(lambda x: filmic_curve(x, spline))
        self._spline, self.parameters = dict(spline, white_ev=asked['white_ev'], output_power=asked['output_power']), spline
        self._install(*tables)

    # ---- the call
    def process(self, image: torch.Tensor, out_dtype: torch.dtype = torch.uint8, out: torch.Tensor | None = None) -> torch.Tensor:
        """(..., 3) float32 or float16 -> the same shape in `out_dtype` (uint8, float16 or float32).  out: a contiguous tensor of that
        shape and type to write into (it may start anywhere in its storage)."""
        if image.dim() < 1 or image.shape[-1] != 3:
            raise ValueError(f'image must have three channels in its last dimension, got shape {tuple(image.shape)}')
        if TAGS.get(image.dtype) not in (TDK_F32, TDK_F16):
            raise ValueError(f'image must be float32 or float16, got {image.dtype}')
        if out_dtype not in TAGS:
            raise ValueError(f'out_dtype must be float32, float16 or uint8, got {out_dtype}')
        _require(image.is_cuda, 'Input must be on CUDA device')
        _require(image.is_contiguous(), 'Input must be contiguous')
        if self._curve is None or self._curve.device != image.device:
            raise RuntimeError(f'Filmic was built for {None if self._curve is None else self._curve.device}, the image is on {image.device}')
        if out is not None:
            if out.dtype != out_dtype or out.shape != image.shape:
                raise ValueError(f'out must be {out_dtype} of shape {tuple(image.shape)}, got {out.dtype} {tuple(out.shape)}')
            _require(out.device == image.device, 'out must be on the image\'s device')
            _require(out.is_contiguous(), 'out must be contiguous')
        with torch.cuda.device(image.device):
            if out is None:
                out = torch.empty(image.shape, dtype=out_dtype, device=image.device)
            if image.numel() == 0:
                return out
            rc = lib.tdk_filmic(_ptr(image), _ptr(out), _ptr(self._curve), _ptr(self._encode), _ptr(self._exposure), image.numel() // 3, TAGS[image.dtype],
                                TAGS[out_dtype], NORMS[self.norm], self._c_weights, 0, _stream())
        check(rc)
        return out


__all__ = ['Filmic']
