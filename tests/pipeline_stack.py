"""What tests/test_gpu_pipeline_stack.py runs ImageProcessor on with its added stages combined, and what tests/test_pipeline_stack.py
checks of it without a GPU: the scene (two cameras, three calls, a bracket of three exposures), the parameters of every stage, the packed
payloads, the chain of the raw half in the NumPy restatements of the stages' headers, and the table of configurations.

No fixture, no test and nothing here touches a GPU at import; `stage` and `processor` build the objects for a caller who has one.

The order the tests pin (ImageProcessor.load_image / load_bracket, then _process_frames):

    decode | raw_correction without gains -> temporal (key: the image name) | hdr (process_bracket) -> chromatic -> highlights | white
    balance -> demosaic (RCD + PostProcess | LMMSE + PostProcess) -> storage type -> chroma_denoise (inside noise_model's transform) ->
    defringe -> capture_sharpen -> color -> dehaze -> tone_equalizer -> bounds (exposure | minimum and maximum) -> process_rgb ->
    metrics -> filmic | the settings' tone mapper -> look -> resize -> sharpen -> orientation

The demosaic turns a mosaic into a frame and the tone mapper a float frame into bytes, so neither can trade places with a neighbour:
the order witnesses are the adjacent pairs on either side of them."""

import collections
import functools
import importlib.util
import itertools
from pathlib import Path

import numpy as np

import chromatic_spec
import hdrmerge_spec
import temporal_spec


def _load(name):
    spec = importlib.util.spec_from_file_location(name.removeprefix('test_'), Path(__file__).resolve().parent / f'{name}.py')
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


rawprepare_spec = _load('test_rawprepare_spec')
highlights_spec = _load('test_highlights_spec')

F = np.float32
W, H = 128, 96                      # even, whole 8-pixel cells, larger than every apron: the size of the per-stage pipeline tests
PATTERN = 'RGGB'
PATTERN_WORD = rawprepare_spec.PATTERNS[PATTERN]
NAMES = ('left', 'right')
TRANSFORMS = {'left': 'rotate_90', 'right': 'flip_horiz'}
CALLS = 3
BRIGHTNESS = (1.0, 1.0, 0.6)        # the third call is darker: the moving averages of bounds and metrics matter
GAINS = (1.9, 1.0, 1.6)
PADDING = 16                        # of every configuration with raw_correction: each branch slices the payload itself
MOVING_AVERAGE = 0.3
RESIZE_WIDTH = 100                  # -> 100 x 75

# ------------------------------------------------------------------ the parameters of the stages
BLACK, WHITE = (64.0, 66.0, 62.0, 65.0), 4095.0
NOISE_A, NOISE_B = (3e-4, 2e-4, 4e-4), 2e-6
NOISE_MODEL = np.array([[a, NOISE_B, 1, 0] for a in NOISE_A], F)        # what NoiseModel.from_values(NOISE_A, NOISE_B) holds
NOISE_SHARE = 0.7                   # the variance of the frames' noise over the model's: a static site stays below t_lo
CA_MODEL = np.array([[1.010, 0.002, -0.001, 1], [0.992, -0.001, 0.002, 1]], F)
MAX_FRAMES = 8.0
EXPOSURES = (1.0, 0.25, 1 / 16)
BRACKET_CALLS = 2
BRACKET_BRIGHTNESS = (1.0, 0.7)


def shading_grid():
    """(5, 9, 4): a lens that darkens towards the corners, a little differently per CFA position."""
    gy, gx = np.meshgrid(np.linspace(-1, 1, 5), np.linspace(-1, 1, 9), indexing='ij')
    r2 = (gx * gx + gy * gy) / 2
    return np.stack([1.0 + k * r2 for k in (0.12, 0.10, 0.10, 0.08)], axis=-1).astype(F)


def stage(td, dev, name, variant=None):
    """A new object of the stage `name` with the parameters of this module (every call gives another instance: the stages that keep
    history between calls must not be shared between the processor and the chain composed by hand)."""
    import torch
    size, pattern = (W, H), td.BayerPattern[PATTERN]
    model = lambda: td.NoiseModel.from_values(NOISE_A, NOISE_B, dev)
    if name == 'raw_correction':
        return td.RawPrepare(dev, size, pattern, black=BLACK, white=WHITE, hot=True, dead=True, shading=torch.from_numpy(shading_grid()))
    if name == 'temporal':
        return td.TemporalDenoise(dev, size, pattern, model(), max_frames=MAX_FRAMES)
    if name == 'hdr':
        return (td.MotionHdrMerge if variant == 'motion' else td.HdrMerge)(dev, size, pattern, model())
    if name == 'chromatic':
        return td.ChromaticAberration(dev, size, pattern, model=torch.from_numpy(CA_MODEL).to(dev))
    if name == 'highlights':
        return td.Highlights(dev, size, pattern)
    if name == 'demosaic':
        return td.LMMSE(dev, size, pattern)
    if name == 'chroma_denoise':
        return td.Wavelet.from_sigma(dev, size, (1.0, 1.0, 1.0), scales=3)
    if name == 'noise_model':
        return model()
    if name == 'defringe':
        return td.Defringe(dev, size, strength=1.0)
    if name == 'capture_sharpen':
        return td.Deconvolve(dev, size, sigma=0.7, iterations=3)
    if name == 'color':
        return td.ColorLUT(dev, matrix=((0.9, 0.1, 0.0), (0.05, 0.9, 0.05), (0.0, 0.2, 0.8)))
    if name == 'dehaze':
        return td.Dehaze(dev, size, quantile=0.05)
    if name == 'tone_equalizer':
        return td.ToneEqualizer(dev, size, gains_ev=(3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0), cell=8, radius=2)
    if name == 'exposure':
        return td.FrameStats(dev, size, bins=1024, value_range=(0.0, 2.0), stride=2, quantiles=(0.01, 0.99), max_frames=len(NAMES))
    if name == 'filmic':
        f = td.Filmic(dev, norm='power')
        f.set_exposure(1.7)
        return f
    if name == 'look':
        return td.ColorLUT(dev, matrix=((1.15, -0.1, -0.05), (-0.05, 1.1, -0.05), (0.0, -0.1, 1.1)), shaper=np.linspace(0.0, 1.0, 64) ** 0.8)
    if name == 'sharpen':
        return td.Sharpen(dev, sigma=1.0, amount=0.8, threshold=0.004, overshoot=0.03)
    raise KeyError(name)


CONSTRUCTOR = ('raw_correction', 'temporal', 'hdr', 'chromatic', 'highlights', 'chroma_denoise', 'noise_model', 'color', 'exposure', 'look', 'sharpen')
PROPERTIES = ('demosaic', 'defringe', 'capture_sharpen', 'dehaze', 'tone_equalizer', 'filmic')


def settings(resize_width=RESIZE_WIDTH):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ToneMapper
    return ImageProcessingSettings(moving_average=MOVING_AVERAGE, postprocess=True, color_smoothing_passes=1, enable_denoise=True, enable_bilateral=True,
                                   tone_mapping=ToneMapper.reinhard, debayer=Debayer.rcd, resize_width=resize_width)


def processor(td, dev, stages, storage='float32', padding=0, resize_width=RESIZE_WIDTH):
    """An ImageProcessor with `stages` ({name: object}; a name left out: no such stage) and the per-camera orientations."""
    import torch
    from torch_darktable.pipeline import ImageProcessor, ImageTransform
    unknown = set(stages) - set(CONSTRUCTOR) - set(PROPERTIES)
    assert not unknown, unknown
    p = ImageProcessor((W, H), td.BayerPattern[PATTERN], td.PackedFormat.Packed12, settings(resize_width), dev, GAINS,
                       transforms={n: ImageTransform[t] for n, t in TRANSFORMS.items()}, padding=padding, storage_dtype=getattr(torch, storage),
                       **{k: v for k, v in stages.items() if k in CONSTRUCTOR})
    for k in PROPERTIES:
        if k in stages:
            setattr(p, k, stages[k])
    return p


# ------------------------------------------------------------------ the table of configurations
RAW_STAGES = ('temporal', 'raw_correction', 'chromatic', 'highlights')
DEMOSAICS = ('rcd', 'lmmse')        # RCD with PostProcess; LMMSE (the stage `demosaic`) with PostProcess
STORAGES = ('float32', 'float16')
RawCase = collections.namedtuple('RawCase', 'temporal raw_correction chromatic highlights demosaic storage padding white_balance_by')


def _white_balance_by(temporal, raw_correction, chromatic, highlights, demosaic):
    """Which operator multiplies by the gains.  `raw_correction` does so only when nothing else stands between it and the demosaic."""
    if highlights:
        return 'highlights'
    if temporal or chromatic:
        return 'apply_white_balance'
    if raw_correction:
        return 'raw_correction'
    return 'fused' if demosaic == 'rcd' else 'apply_white_balance'   # decode + white balance + RCD in one kernel


RAW_CASES = [RawCase(*on, demosaic, storage, PADDING if on[1] else 0, _white_balance_by(*on, demosaic))
             for demosaic in DEMOSAICS for storage in STORAGES for on in itertools.product((False, True), repeat=len(RAW_STAGES))]


def raw_cases(demosaic, storage):
    return [c for c in RAW_CASES if c.demosaic == demosaic and c.storage == storage]


def case_id(c):
    return '+'.join(n for n in RAW_STAGES if getattr(c, n)) or 'none'


FRAME_STAGES = ('chroma_denoise', 'defringe', 'capture_sharpen', 'color', 'dehaze', 'tone_equalizer')    # in the order _process_frames runs them
# everything that combines on a sequence (section 3), and on a bracket (section 4); `resize_width` is a field of the settings
FULL_STACK = ('raw_correction', 'temporal', 'chromatic', 'highlights', 'demosaic', 'chroma_denoise', 'noise_model', 'defringe', 'capture_sharpen', 'color',
              'dehaze', 'tone_equalizer', 'exposure', 'filmic', 'look', 'resize_width', 'sharpen')
BRACKET_STACK = tuple('hdr' if n == 'temporal' else n for n in FULL_STACK)
# the arguments of ImageProcessor.__init__ that are no stage
PLUMBING = ('self', 'image_size', 'bayer_pattern', 'packed_format', 'settings', 'device', 'white_balance', 'transforms', 'padding', 'storage_dtype')


def covered():
    """Every stage name that some configuration of this module switches on."""
    return set(FULL_STACK) | set(BRACKET_STACK) | {n for c in RAW_CASES for n in RAW_STAGES if getattr(c, n)} | {'demosaic'}


def stage_names_of(processor_class):
    """The stage names of ImageProcessor as `inspect` finds them: the constructor's arguments that are no plumbing, and the properties
    with a setter."""
    import inspect
    arguments = [n for n in inspect.signature(processor_class.__init__).parameters if n not in PLUMBING]
    properties = [n for n, v in inspect.getmembers(processor_class, lambda v: isinstance(v, property)) if v.fset is not None]
    return arguments, properties


# ------------------------------------------------------------------ the scene
def _cfa(shape):
    i, j = np.indices(shape)
    return 2 * (i & 1) + (j & 1)


def radiance(shift=0, scale=1.0, blob=3.0):
    """The clean linear mosaic, 1.0 = white level, not yet clipped: a smooth field with fine texture (edges for the sharpeners and
    the fringe detector), a dark bar with hard edges, and two blobs of white light that saturate all three colours at every
    brightness used here."""
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    j = j - shift
    field = 0.34 + 0.16 * np.sin(i / 7.0 + 0.4) * np.cos(j / 11.0) + 0.05 * np.sin(0.9 * j + 0.5 * i)
    field = np.where((i >= 50) & (i < 62) & (j >= 10) & (j < 34), 0.25 * field, field)
    plane = np.array([0.55, 1.0, 1.0, 0.70])[_cfa((H, W))]            # the sensor's colour response: roughly 1 / GAINS
    blobs = blob * np.exp(-((i - 30) ** 2 + (j - 40) ** 2) / (2 * 6.0 ** 2)) + blob * np.exp(-((i - 70) ** 2 + (j - 100) ** 2) / (2 * 5.0 ** 2))
    return scale * (field * plane + blobs)


DEFECTS = {'left': (((20, 70), (57, 20), (84, 33)), ((12, 101), (41, 77))), 'right': (((22, 15), (56, 25), (80, 60)), ((15, 90), (44, 60)))}   # (hot, dead)


def _codes(clean, seed, defects=((), ())):
    """A clean linear mosaic -> the 12-bit codes of a sensor with the black levels, the white level and a share of the model's noise."""
    rng = np.random.default_rng(seed)
    colour = np.array([0, 1, 1, 2])[_cfa(clean.shape)]
    var = NOISE_SHARE * (np.asarray(NOISE_A)[colour] * np.clip(clean, 0, 1) + NOISE_B)
    noisy = clean + rng.standard_normal(clean.shape) * np.sqrt(var)
    black = np.asarray(BLACK)[_cfa(clean.shape)]
    codes = np.clip(np.rint(black + noisy * (WHITE - black)), 0, 4095).astype(np.uint16)
    for i, j in defects[0]:
        codes[i, j] = 4000
    for i, j in defects[1]:
        codes[i, j] = 70
    return codes


@functools.lru_cache(maxsize=None)
def codes(name, call):
    """(H, W) uint16: the frame of camera `name` at call `call`.  The second camera sees the scene six sites to the side."""
    k = NAMES.index(name)
    return _codes(radiance(shift=6 * k, scale=BRIGHTNESS[call]), 1000 + 10 * k + call, DEFECTS[name])


@functools.lru_cache(maxsize=None)
def bracket_codes(call):
    """The three exposures of bracket `call`: a scene of three times the range, of which the longest frame clips more than a tenth, with
    lights that clip the shortest frame too (the merge is in its units: they are the highlight stage's share); the middle frame is
    two sites to the side (whole CFA cells: something for the aligned merge to find, a ghost for the plain one to reject)."""
    scene = radiance(scale=3.0 * BRACKET_BRIGHTNESS[call], blob=12.0)
    frames = [_codes(scene * e, 2000 + 10 * call + f) for f, e in enumerate(EXPOSURES)]
    frames[1] = np.roll(frames[1], 2, axis=1)
    return tuple(frames)


def payload(frame, padding=0):
    """Packed12 bytes of a frame of codes, with `padding` bytes that are not zero behind them."""
    return np.concatenate([rawprepare_spec.pack12(frame, False), np.arange(1, padding + 1, dtype=np.uint8)])


# ------------------------------------------------------------------ the raw half in the restatements
def geometry():
    """(x0, y0, rn) of the chromatic stage: the defaults of ChromaticAberration for this size."""
    return chromatic_spec.default_geometry(W, H)


def prepared(frame):
    """raw_correction without gains: tests/test_rawprepare_spec.py's restatement on the unpacked codes."""
    black, scale = rawprepare_spec.scale_of(BLACK, WHITE)
    return rawprepare_spec.raw_prepare_ref(frame, PATTERN_WORD, black, scale, hot=True, dead=True, shading=shading_grid(), gains=None, clip=True)[0]


def decoded(frame):
    """The plain decode: code * (1 / 4095) in float32."""
    return frame.astype(F) * (F(1.0) / F(4095.0))


def corrected(mosaic):
    return chromatic_spec.correct(mosaic, chromatic_spec.PATTERNS[PATTERN], CA_MODEL, *geometry(), chromatic_spec.BILINEAR)


def balanced(mosaic):
    """The highlight stage: (the mosaic the demosaic gets, sum, cnt, chroma)."""
    return highlights_spec.highlights_ref(mosaic, GAINS, highlights_spec.PATTERNS[PATTERN])


def sequence_chain(name, state=None):
    """The three calls of camera `name` with all four raw stages on: per call (prepared, filtered, corrected, balanced), float32 (H, W)
    each, the last being what `_demosaic` is given.  `state`: a temporal_spec.State to use and leave advanced."""
    state = temporal_spec.State((H, W)) if state is None else state
    out = []
    for call in range(CALLS):
        a = prepared(codes(name, call))
        b = temporal_spec.step(a, state, NOISE_MODEL, temporal_spec.RGGB, max_frames=MAX_FRAMES)
        c = corrected(b)
        out.append((a, b, c, balanced(c)[0]))
    return out


def bracket_chain(call):
    """Bracket `call` with raw_correction, the plain merge, chromatic and highlights: (prepared frames, merged, corrected, balanced)."""
    frames = [prepared(f) for f in bracket_codes(call)]
    merged = hdrmerge_spec.merge(frames, EXPOSURES, NOISE_MODEL, hdrmerge_spec.RGGB)[0]
    c = corrected(merged)
    return frames, merged, c, balanced(c)[0]


def bits(a):
    """The bit patterns of a float array, with every NaN as one pattern: which NaN an operation returns is not specified."""
    a = np.ascontiguousarray(a)
    out = a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize]).copy()
    out[np.isnan(a)] = -1
    return out
