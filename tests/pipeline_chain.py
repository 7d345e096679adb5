"""The oracle's restatement of ImageProcessor._process_image_set, and the configurations the pipeline tests run.

`oracle_chain` spells one call of `process_image_set` on the CPU oracle's functions (numpy + tdk_oracle, no torch):
decode12 -> white balance -> demosaic -> [post-process] -> bounds over the set -> EMA -> normalise -> [Wiener on log-luminance] ->
[bilateral] -> metrics over the set -> EMA -> tonemap -> orientation, with the fp32 EMA arithmetic of
tests/test_gpu_next_rows.py::test_process_image_set_shared_bounds_and_ema part (b).  Every intermediate is returned, so that a test
can compare stage by stage.

The reference's adaptive mappers (reinhard, linear, adaptive_aces) are discontinuous at a zero channel when light_adapt == 1
(oracle/src/color_ops.c, tonemap_pixel: adapt = pow(rgb / exposure, key) is 0, the mapper divides by it, and for adaptive_aces the
NaN blackens the whole pixel).  `ill_conditioned` marks the pixels where an end-to-end uint8 comparison goes through that
discontinuity; tests/test_pipeline_chain.py measures, on the oracle alone, that everything outside the mask is well conditioned.

CONFIGS: A the shipped presets, B the reference camera files at a small frame size, C a hand-written table over the settings that
select a branch of load_image / process_rgb / tonemap / transform, D float16 storage."""

from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import torch  # the storage dtype of a Config only; the chain below is numpy

TOL = 2e-5  # the colour operators' tolerance, the TOL of tests/test_gpu_lab_chain.py

SMALL = (132, 74)    # (w, h): the fused-head test's size, several Wiener and bilateral tiles with tails on both axes
SMALL_B = (128, 96)  # the size of the two existing ImageProcessor tests

TRANSFORMS = ['none', 'rotate_90', 'rotate_180', 'rotate_270', 'transpose', 'flip_horiz', 'flip_vert', 'transverse']
STAGES = {'both': (True, True), 'denoise': (True, False), 'bilateral': (False, True), 'neither': (False, False)}
ADAPTIVE = ('reinhard', 'linear', 'adaptive_aces')   # the mappers that divide by `adapt`


@dataclass(frozen=True)
class Config:
    name: str
    group: str                                # 'A' | 'B' | 'C' | 'D'
    settings: object                          # ImageProcessingSettings
    pattern: str = 'RGGB'
    packed_format: str = 'Packed12'           # | 'Packed12_IDS'
    padding: int = 0
    white_balance: tuple | None = None
    transform: object = 'none'                # an ImageTransform name, or {image name: ImageTransform name}
    storage_dtype: torch.dtype = torch.float32
    size: tuple = SMALL                       # (w, h)
    names: tuple = ('cam',)                   # the image set of one call
    calls: int = 1                            # the second call's set is darker: the EMA, not the fresh statistics, decides
    seed: int = 300
    camera: object = field(default=None, compare=False)   # group B: the CameraSettings the processor is built from

    @property
    def ids(self) -> bool:
        return self.packed_format == 'Packed12_IDS'

    @property
    def stages(self) -> str:
        return {v: k for k, v in STAGES.items()}[(bool(self.settings.enable_denoise), bool(self.settings.enable_bilateral))]

    def transform_of(self, image_name: str) -> str:
        return self.transform[image_name] if isinstance(self.transform, dict) else self.transform

    @property
    def green_bound(self) -> float:
        """Relative bound on what the global green equilibration may differ by (tests/test_gpu_parity.py::
        test_postprocess_global_green_eq: two fp32 sums of H W / 4 terms in different association orders)."""
        w, h = self.size
        blocks = ((h + 15) // 16) * ((w + 15) // 16)
        return 2.0 * ((8 + blocks) + (8 + 12)) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- inputs
def frames(oracle, scene, cfg: Config, call: int) -> dict:
    """{image name: packed bytes + padding} of one call.  The padding bytes are not zero: they must be cut off, not decoded."""
    w, h = cfg.size
    pat = oracle.PATTERNS[cfg.pattern]
    out = {}
    for i, name in enumerate(cfg.names):
        gain = (1.0, 0.75)[call] * (0.85 + 0.15 * i)
        bayer = np.clip(oracle.mosaic(scene(h, w, cfg.seed + 10 * call + i) * gain, pat)[:, :, 0], 0, 1)
        packed = oracle.encode12_f32(bayer.ravel(), cfg.ids, True)
        out[name] = np.concatenate([packed, np.full(cfg.padding, 0xA5, np.uint8)])
    return out


# ---------------------------------------------------------------------------------------------------------------- the chain
def _r16(a: np.ndarray) -> np.ndarray:
    return a.astype(np.float16).astype(np.float32)


def orient(img: np.ndarray, transform: str) -> np.ndarray:
    rot = {'rotate_90': 1, 'rotate_180': 2, 'rotate_270': 3}
    if transform == 'none':
        return img
    if transform in rot:
        return np.rot90(img, rot[transform], (0, 1))
    if transform == 'flip_horiz':
        return img[:, ::-1]
    if transform == 'flip_vert':
        return img[::-1]
    if transform == 'transverse':
        return img[::-1, ::-1]
    assert transform == 'transpose', transform
    return np.swapaxes(img, 0, 1)


def demosaic(oracle, cfg: Config, packed: np.ndarray, half: bool = False) -> np.ndarray:
    s, pat = cfg.settings, oracle.PATTERNS[cfg.pattern]
    w, h = cfg.size
    payload = packed[: packed.size - cfg.padding] if cfg.padding > 0 else packed
    bayer = oracle.decode12_f32(payload, cfg.ids, True).reshape(h, w)
    if cfg.white_balance is not None:
        bayer = oracle.apply_white_balance(bayer, list(cfg.white_balance), pat)
    if s.debayer.name == 'rcd':
        rgb = oracle.rcd(bayer, pat)
        if half and s.postprocess:   # the fused head stores its result in the storage type, the post-process reads that
            rgb = _r16(rgb)
    elif s.debayer.name == 'ppg':
        rgb = oracle.ppg(bayer, pat, s.ppg_median_threshold)
    else:
        rgb = oracle.bilinear5x5(bayer, pat)
    if s.postprocess:
        rgb = oracle.postprocess(rgb, pat, s.color_smoothing_passes, False, True, s.green_eq_threshold)
    return _r16(rgb) if half else rgb


def tonemap(oracle, cfg: Config, pre: np.ndarray, metrics: np.ndarray) -> np.ndarray:
    s = cfg.settings
    return oracle.tonemap(s.tone_mapping.name, pre, metrics, s.tone_gamma, s.tone_intensity, s.light_adapt, s.vibrance)


def _ema(prev, new, t):
    # pipeline.util.lerp in fp32: a + (b - a) * t, with a = b on the first call
    f = np.float32
    prev = new if prev is None else prev
    return (prev + (new - prev) * f(t)).astype(f)


def oracle_chain(oracle, cfg: Config, packed_by_name: dict, state: dict, half: bool = False) -> dict:
    """One call of process_image_set.  `state` carries the moving averages of bounds and metrics across calls.  half: the images are
    rounded to binary16 where a float16 processor stores them (after the fused RCD head in front of a post-process, after demosaic /
    post-process, after normalise when the first stage does not fuse it, after process_rgb); the arithmetic stays fp32."""
    f, s = np.float32, cfg.settings
    denoise, bilateral = STAGES[cfg.stages]
    rgb = {n: demosaic(oracle, cfg, p, half) for n, p in packed_by_name.items()}
    state['bounds'] = bounds = _ema(state.get('bounds'), oracle.image_bounds(list(rgb.values()), 8), s.moving_average)
    pre = {}
    for n, img in rgb.items():
        x = ((img - bounds[0]) / (bounds[1] - bounds[0])).astype(f)
        if half and not (denoise and bilateral):
            x = _r16(x)
        if denoise:
            ll = oracle.compute_luminance(x, True, 1e-4)
            x = oracle.modify_luminance(x, oracle.wiener(ll[:, :, None], s.denoise, 32, 4)[:, :, 0], True)
        if bilateral:
            x = oracle.modify_luminance(x, oracle.bilateral(oracle.compute_luminance(x), s.bil_sigma_spatial, s.bil_sigma_luminance, s.bilateral))
        pre[n] = _r16(x) if half else x
    state['metrics'] = metrics = _ema(state.get('metrics'), oracle.image_metrics(list(pre.values()), 8), s.moving_average)
    u8 = {n: tonemap(oracle, cfg, x, metrics) for n, x in pre.items()}
    out = {n: np.ascontiguousarray(orient(img, cfg.transform_of(n))) for n, img in u8.items()}
    return dict(demosaiced=rgb, bounds=bounds.copy(), pre=pre, metrics=metrics.copy(), u8=u8, out=out)


_cache: dict = {}


def reference(oracle, scene, cfg: Config, half: bool = False) -> list:
    """[(packed_by_name, oracle_chain result) per call], computed once per configuration and left unchanged."""
    key = (cfg.name, half)
    if key not in _cache:
        state, calls = {}, []
        for call in range(cfg.calls):
            packed = frames(oracle, scene, cfg, call)
            calls.append((packed, oracle_chain(oracle, cfg, packed, state, half)))
        _cache[key] = calls
    return _cache[key]


def f16_measure(oracle, scene, cfg: Config) -> tuple:
    """(largest uint8 difference, share of values above 1 LSB) between the oracle chain in float32 and the same chain with the images
    rounded to binary16 where a float16 processor stores them, over every frame of every call."""
    d = np.concatenate([np.abs(a['out'][n].astype(np.int32) - b['out'][n].astype(np.int32)).ravel()
                        for (_, a), (_, b) in zip(reference(oracle, scene, cfg), reference(oracle, scene, cfg, half=True)) for n in cfg.names])
    return int(d.max()), float((d > 1).mean())


def f16_bound(oracle, scene, cfg: Config) -> tuple:
    """What a float16 processor may differ from the float32 oracle chain by: (max, share above 1 LSB).  The reference's own figure,
    plus 1 LSB, and twice its share: the margin for positions where a rounded value flips a median or a bilateral cell differently."""
    worst, share = f16_measure(oracle, scene, cfg)
    worst, share = worst + 1, 2.0 * share
    if cfg.name in F16_ALREADY_BOUNDED:   # never looser than what the suite already holds this configuration to
        worst, share = min(worst, F16_ALREADY_BOUNDED[cfg.name][0]), min(share, F16_ALREADY_BOUNDED[cfg.name][1])
    return worst, share


def ill_conditioned(cfg: Config, pre: np.ndarray) -> np.ndarray:
    """(H, W) bool: the pixels of the oracle's pre-tonemap image at which the mapper of `cfg` is discontinuous."""
    s = cfg.settings
    if s.tone_mapping.name not in ADAPTIVE or s.light_adapt != 1.0:
        return np.zeros(pre.shape[:2], bool)
    return (pre <= 2 * TOL).any(axis=-1)


# ---------------------------------------------------------------------------------------------------------------- configurations
def _settings(**kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ToneMapper

    kw['debayer'] = Debayer[kw.pop('debayer', 'rcd')]
    kw['tone_mapping'] = ToneMapper[kw.pop('mapper', 'reinhard')]
    den, bil = STAGES[kw.pop('stages', 'denoise')]
    return ImageProcessingSettings(enable_denoise=den, enable_bilateral=bil, **kw)


# C: debayer, postprocess, stages, mapper, pattern, gains, format, padding, transform, light_adapt (1.0 is the settings' default).
# tests/test_pipeline_chain.py::test_table_covers_its_pairs holds the coverage this table is written for.
_GAINS = (1.9, 1.0, 1.45)
TABLE_C = [
    ('bilinear', False, 'both',      'linear',        'RGGB', _GAINS, 'Packed12',     0,  'none',       0.8),
    ('ppg',      True,  'both',      'reinhard',      'BGGR', None,   'Packed12_IDS', 64, 'rotate_90',  0.8),
    ('rcd',      False, 'both',      'aces',          'GRBG', None,   'Packed12',     0,  'rotate_180', 0.8),
    ('rcd',      True,  'both',      'adaptive_aces', 'GBRG', _GAINS, 'Packed12_IDS', 64, 'rotate_270', 1.0),
    ('ppg',      False, 'denoise',   'linear',        'RGGB', _GAINS, 'Packed12',     64, 'transpose',  0.8),   # ppg_median_threshold > 0
    ('rcd',      False, 'denoise',   'reinhard',      'BGGR', _GAINS, 'Packed12',     0,  'flip_horiz', 1.0),
    ('bilinear', True,  'denoise',   'aces',          'GRBG', None,   'Packed12_IDS', 0,  'flip_vert',  0.8),
    ('ppg',      True,  'denoise',   'adaptive_aces', 'GBRG', _GAINS, 'Packed12',     0,  'transverse', 0.8),
    ('rcd',      True,  'bilateral', 'linear',        'RGGB', None,   'Packed12',     64, 'none',       1.0),
    ('bilinear', False, 'bilateral', 'reinhard',      'BGGR', _GAINS, 'Packed12_IDS', 0,  'rotate_90',  0.8),
    ('ppg',      False, 'bilateral', 'aces',          'GRBG', _GAINS, 'Packed12',     0,  'rotate_270', 0.8),
    ('bilinear', True,  'bilateral', 'adaptive_aces', 'GBRG', _GAINS, 'Packed12',     64, 'transpose',  0.8),
    ('rcd',      False, 'neither',   'linear',        'GRBG', None,   'Packed12_IDS', 0,  'flip_horiz', 0.8),
    ('ppg',      False, 'neither',   'reinhard',      'RGGB', _GAINS, 'Packed12',     64, 'flip_vert',  0.8),
    ('bilinear', False, 'neither',   'aces',          'BGGR', None,   'Packed12',     0,  'transverse', 0.8),
    ('rcd',      True,  'neither',   'adaptive_aces', 'GBRG', _GAINS, 'Packed12_IDS', 64, 'rotate_180', 0.8),
]
_C_LARGER = (2,)     # rows of C at SMALL_B
# reinhard at light_adapt = 1 is steep just above a zero channel as well: scene 415 has a channel of a few 1e-5, outside the mask, that
# +-2 TOL moves by 2 LSB (tests/test_pipeline_chain.py::test_reference_conditions); scene 505 has no value in (2 TOL, 1e-3)
_C_SEEDS = {5: 505}
# what binary16 storage does to the oracle chain itself depends on the scene (aces preset, scenes 310 .. 325: 1 to 11 LSB, where a rounded
# value flips a colour-smoothing median).  The configuration the suite already bounds (F16_ALREADY_BOUNDED) runs on a scene where the
# reference's own figure plus 1 LSB stays inside that bound: tests/test_pipeline_chain.py::test_float16_bound_from_the_reference
_D_SEEDS = {'D-aces': 320}
_D_ROWS = (1, 3, 9)  # rows of C that also run with float16 storage: ppg + post-process, the fused RCD head, bilinear + one stage


def _row_name(i: int, row) -> str:
    deb, post, stages, mapper, pattern, gains, fmt, pad, tf, la = row
    return f'C{i:02d}-{deb}{"+pp" if post else ""}-{stages}-{mapper}-{pattern}'


def _row_config(i: int, row, **kw) -> Config:
    deb, post, stages, mapper, pattern, gains, fmt, pad, tf, la = row
    s = _settings(debayer=deb, postprocess=post, stages=stages, mapper=mapper, light_adapt=la, moving_average=1.0, tone_gamma=2.2, tone_intensity=1.0,
                  vibrance=0.3, ppg_median_threshold=0.02 if i == 4 else 0.0)
    base = dict(name=_row_name(i, row), group='C', settings=s, pattern=pattern, packed_format=fmt, padding=pad, white_balance=gains, transform=tf,
                size=SMALL_B if i in _C_LARGER else SMALL, seed=_C_SEEDS.get(i, 400 + 3 * i))
    base.update(kw)
    return Config(**base)


def _build_configs() -> list:
    # the settings classes live in the product package, whose import loads the kernel library: as the `td` fixture, at collection
    import __graft_entry__

    __graft_entry__.ensure_built()
    from torch_darktable.pipeline import CameraSettings, presets

    configs = []
    # A: the presets as shipped
    for k, (name, s) in enumerate(presets.items()):
        configs.append(Config(name=f'A-{name}', group='A', settings=s.model_copy(update={'moving_average': 1.0}), white_balance=(1.5, 1.0, 1.2),
                              size=SMALL_B if name == 'aces' else SMALL, seed=310 + 3 * k))
    # B: the reference camera files; only image_size is replaced
    for k, path in enumerate(sorted((Path(__file__).parent / 'golden' / 'camera_settings').glob('*.json'))):
        cs = CameraSettings.load_json(path)
        cs = cs.model_copy(update={'image_size': SMALL_B if cs.name == 'pfr' else SMALL})
        if isinstance(cs.transform, dict):
            tf, names = {n: t.name for n, t in cs.transform.items()}, ('cam1', 'cam7')
            assert tf['cam1'] != tf['cam7']
        else:
            tf, names = cs.transform.name, ('cam1', 'cam2')
        configs.append(Config(name=f'B-{cs.name}', group='B', settings=cs.image_processing, pattern=cs.bayer_pattern.name, packed_format=cs.packed_format.name,
                              padding=cs.padding, white_balance=cs.white_balance, transform=tf, size=tuple(cs.image_size), names=names, calls=2,
                              seed=340 + 20 * k, camera=cs))
    # C: the table
    configs += [_row_config(i, row) for i, row in enumerate(TABLE_C)]
    # D: float16 storage
    for c in [c for c in configs if c.group == 'A']:
        name = c.name.replace('A-', 'D-')
        configs.append(Config(**{**c.__dict__, 'name': name, 'group': 'D', 'storage_dtype': torch.float16, 'seed': _D_SEEDS.get(name, c.seed)}))
    for i in _D_ROWS:
        configs.append(_row_config(i, TABLE_C[i], name=_row_name(i, TABLE_C[i]).replace('C', 'D', 1), group='D', storage_dtype=torch.float16))
    assert len({c.name for c in configs}) == len(configs)
    return configs


CONFIGS = _build_configs()
F32_CONFIGS = [c for c in CONFIGS if c.storage_dtype == torch.float32]
F16_CONFIGS = [c for c in CONFIGS if c.storage_dtype == torch.float16]
# the float16 configuration tests/test_gpu_parity.py::test_image_processor_end_to_end already bounds (RGGB, Packed12, RCD + post-process,
# both stages, ACES, 128 x 96): max <= 4, share(> 1 LSB) < 5e-4
F16_ALREADY_BOUNDED = {'D-aces': (4, 5e-4)}
