"""The refusals and reprs of the stages on raw (H, W) mosaics, as a table: RawPrepare, Highlights, ChromaticAberration, NoiseProfile
(with NoiseModel's transform), TemporalDenoise, MotionEstimate, MotionTemporalDenoise, HdrMerge, MotionHdrMerge, FrameStats, and the
slots of ImageProcessor that take them.  Every message is written out by hand from the sources and matched whole.  Everything here is
reached without a GPU: an object is built for cuda:0 and never run, and a call gets CPU tensors, so the last row of a call is always
'Input must be on CUDA device'.  What only a CUDA tensor reaches is in test_gpu_mosaic_refusals.py.

A row of CONSTRUCT is (class, arguments that replace those of BASE, exception, message); of REPRS (class, arguments, repr); of CALLS
(class, constructor arguments, method, positional arguments, keyword arguments, exception, message).  `New` stands for an object the
walker builds, `PATTERN` and `MODEL` for a BayerPattern and a NoiseModel; a row with two wrong arguments fixes which one is named."""

import math

import torch

DEVICE = torch.device('cuda', 0)
CPU = torch.device('cpu')
SIZE = (16, 8)      # (width, height): frames are (8, 16)
NAN, INF = math.nan, math.inf


class New:
    """An object of the package the walker builds: New('MotionEstimate', image_size=(32, 8))."""

    def __init__(self, cls: str, **kwargs):
        self.cls, self.kwargs = cls, kwargs


PATTERN = New('BayerPattern.RGGB')
MODEL = New('NoiseModel', model=torch.zeros(3, 4))


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


FRAME, HALF, SMALL = z(8, 16), z(8, 16, dtype=torch.float16), z(8, 8)

BASE = {
    'RawPrepare': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN),
    'Highlights': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN),
    'ChromaticAberration': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN),
    'ChromaticAberration.from_coefficients': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN),
    'NoiseProfile': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN),
    'NoiseModel': dict(model=torch.zeros(3, 4)),
    'TemporalDenoise': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN, noise_model=MODEL),
    'MotionEstimate': dict(device=DEVICE, image_size=SIZE),
    'MotionTemporalDenoise': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN, noise_model=MODEL),
    'HdrMerge': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN, noise_model=MODEL),
    'MotionHdrMerge': dict(device=DEVICE, image_size=SIZE, bayer_pattern=PATTERN, noise_model=MODEL),
    'FrameStats': dict(device=DEVICE, image_size=SIZE),
    'ImageProcessor': dict(image_size=SIZE, bayer_pattern=PATTERN, packed_format=None, settings=None, device=DEVICE, white_balance=None),
}

V, T, R, K, A = ValueError, TypeError, RuntimeError, KeyError, AssertionError
DEVICE_MSG = 'Device must be CUDA, got cpu'
RANGE_MSG = 'Image dimensions must be 2..65535, got {}'
PATTERN_MSG = 'Invalid bayer pattern: RGGB'
MOSAIC_EVEN = 'Mosaic dimensions must be even (whole CFA cells), got {}'
IMAGE_EVEN = 'Image dimensions must be even (whole CFA cells), got {}'
RADIUS_MSG = 'radius must be 2 or 3, got {}'
CUDA_MSG = 'Input must be on CUDA device'
OUT_DTYPE_MSG = 'out_dtype must be float32 or float16, got torch.float64'


def _size_rows(cls, even, pattern_first, pattern=True):
    """The rows every stage has: device, range, pattern and whole cells, alone and in pairs, in the stage's order."""
    rows = [(cls, dict(device=CPU), V, DEVICE_MSG),
            (cls, dict(device=CPU, image_size=(0, 8)), V, DEVICE_MSG),
            (cls, dict(image_size=(0, 8)), V, RANGE_MSG.format('0x8')),
            (cls, dict(image_size=(1, 8)), V, RANGE_MSG.format('1x8')),
            (cls, dict(image_size=(16, 1)), V, RANGE_MSG.format('16x1')),
            (cls, dict(image_size=(65536, 8)), V, RANGE_MSG.format('65536x8')),
            (cls, dict(image_size=(16, 65537)), V, RANGE_MSG.format('16x65537')),
            (cls, dict(image_size=(15, 8)), V, even.format('15x8')),
            (cls, dict(image_size=(16, 7)), V, even.format('16x7')),
            (cls, dict(image_size=(65535, 8)), V, even.format('65535x8'))]
    if pattern:
        rows += [(cls, dict(bayer_pattern='RGGB'), V, PATTERN_MSG),
                 (cls, dict(bayer_pattern=0), V, 'Invalid bayer pattern: 0'),
                 (cls, dict(image_size=(1, 8), bayer_pattern='RGGB'), V, RANGE_MSG.format('1x8')),
                 (cls, dict(image_size=(15, 8), bayer_pattern='RGGB'), V, PATTERN_MSG if pattern_first else even.format('15x8'))]
    return rows


def _window_rows(cls):
    """The window statistic of TemporalDenoise and HdrMerge: radius, thresholds and pixel_threshold, variance_floor, noise_model."""
    return [(cls, dict(radius=1), V, RADIUS_MSG.format(1)),
            (cls, dict(radius=4), V, RADIUS_MSG.format(4)),
            (cls, dict(radius=True), V, RADIUS_MSG.format(True)),
            (cls, dict(radius=2.5), V, RADIUS_MSG.format(2.5)),
            (cls, dict(image_size=(16, 7), radius=1), V, MOSAIC_EVEN.format('16x7')),
            (cls, dict(thresholds=(1, 2, 3)), V, 'thresholds must be (t_lo, t_hi), got (1, 2, 3)'),
            (cls, dict(thresholds=(3.0, 1.5)), V, 'thresholds must be finite with 0 < t_lo < t_hi, got (3.0, 1.5)'),
            (cls, dict(thresholds=[0, 1]), V, 'thresholds must be finite with 0 < t_lo < t_hi, got (0, 1)'),
            (cls, dict(thresholds=(1.0, INF)), V, 'thresholds must be finite with 0 < t_lo < t_hi, got (1.0, inf)'),
            (cls, dict(thresholds=(NAN, 3.0)), V, 'thresholds must be finite with 0 < t_lo < t_hi, got (nan, 3.0)'),
            (cls, dict(thresholds=(1.0, 1.0 + 1e-9)), V, 'thresholds must be finite with 0 < t_lo < t_hi, got (1.0, 1.000000001)'),
            (cls, dict(thresholds=(1e-45, 2e-45)), V, 'thresholds must be finite with 0 < t_lo < t_hi, got (1e-45, 2e-45)'),
            (cls, dict(thresholds=(1,), pixel_threshold=0), V, 'thresholds must be (t_lo, t_hi), got (1,)'),
            (cls, dict(thresholds=(2, 1), pixel_threshold=0), V, 'thresholds must be finite with 0 < t_lo < t_hi, got (2, 1)'),
            (cls, dict(pixel_threshold=0), V, 'pixel_threshold must be finite and > 0, or None, got 0'),
            (cls, dict(pixel_threshold=-4.0), V, 'pixel_threshold must be finite and > 0, or None, got -4.0'),
            (cls, dict(pixel_threshold=NAN), V, 'pixel_threshold must be finite and > 0, or None, got nan'),
            (cls, dict(pixel_threshold=INF), V, 'pixel_threshold must be finite and > 0, or None, got inf'),
            (cls, dict(pixel_threshold=1e-30), V, 'pixel_threshold must be finite and > 0, or None, got 1e-30'),
            (cls, dict(variance_floor=0), V, 'variance_floor must be finite and > 0, got 0'),
            (cls, dict(variance_floor=1e-50), V, 'variance_floor must be finite and > 0, got 1e-50'),
            (cls, dict(variance_floor=INF), V, 'variance_floor must be finite and > 0, got inf'),
            (cls, dict(variance_floor=0, noise_model=None), V, 'variance_floor must be finite and > 0, got 0'),
            (cls, dict(noise_model=None), T, 'noise_model must be a NoiseModel, got NoneType'),
            (cls, dict(noise_model=torch.zeros(3, 4)), T, 'noise_model must be a NoiseModel, got Tensor')]


CONSTRUCT = [
    # ---- TemporalDenoise: range, pattern, even; radius, thresholds, pixel_threshold, max_frames, variance_floor, state_dtype, model
    *_size_rows('TemporalDenoise', MOSAIC_EVEN, pattern_first=True),
    *_window_rows('TemporalDenoise'),
    ('TemporalDenoise', dict(radius=5, thresholds=(1,)), V, RADIUS_MSG.format(5)),
    ('TemporalDenoise', dict(max_frames=0.5), V, 'max_frames must be in 1..64, got 0.5'),
    ('TemporalDenoise', dict(max_frames=65), V, 'max_frames must be in 1..64, got 65'),
    ('TemporalDenoise', dict(max_frames=NAN), V, 'max_frames must be in 1..64, got nan'),
    ('TemporalDenoise', dict(pixel_threshold=0, max_frames=0), V, 'pixel_threshold must be finite and > 0, or None, got 0'),
    ('TemporalDenoise', dict(max_frames=0, variance_floor=0), V, 'max_frames must be in 1..64, got 0'),
    ('TemporalDenoise', dict(state_dtype=torch.float64), V, 'state_dtype must be float32 or float16, got torch.float64'),
    ('TemporalDenoise', dict(variance_floor=-1, state_dtype=torch.bfloat16), V, 'variance_floor must be finite and > 0, got -1'),
    ('TemporalDenoise', dict(state_dtype=torch.uint8, noise_model=None), V, 'state_dtype must be float32 or float16, got torch.uint8'),
    # ---- MotionTemporalDenoise: motion first (a default one is built from device and size alone), then the base's
    *_window_rows('MotionTemporalDenoise'),
    ('MotionTemporalDenoise', dict(device=CPU), V, DEVICE_MSG),
    ('MotionTemporalDenoise', dict(image_size=(1, 8)), V, RANGE_MSG.format('1x8')),
    ('MotionTemporalDenoise', dict(bayer_pattern='RGGB'), V, PATTERN_MSG),
    ('MotionTemporalDenoise', dict(image_size=(15, 8)), V, MOSAIC_EVEN.format('15x8')),
    ('MotionTemporalDenoise', dict(image_size=(15, 8), bayer_pattern='RGGB'), V, MOSAIC_EVEN.format('15x8')),   # (the default MotionEstimate)
    ('MotionTemporalDenoise', dict(image_size=(15, 8), bayer_pattern='RGGB', motion=New('MotionEstimate', image_size=(14, 8))), V,
     'motion is for (14, 8), the filter for (15, 8)'),
    ('MotionTemporalDenoise', dict(motion='x'), T, 'motion must be a MotionEstimate, got str'),
    ('MotionTemporalDenoise', dict(device=CPU, motion='x'), T, 'motion must be a MotionEstimate, got str'),
    ('MotionTemporalDenoise', dict(motion=New('MotionEstimate', image_size=(32, 8))), V, 'motion is for (32, 8), the filter for (16, 8)'),
    ('MotionTemporalDenoise', dict(image_size=[16, 8], motion=New('MotionEstimate', image_size=(32, 8))), V, 'motion is for (32, 8), the filter for (16, 8)'),
    ('MotionTemporalDenoise', dict(radius=1, motion=New('MotionEstimate', image_size=(32, 8))), V, 'motion is for (32, 8), the filter for (16, 8)'),
    ('MotionTemporalDenoise', dict(max_frames=65, motion=New('MotionEstimate')), V, 'max_frames must be in 1..64, got 65'),
    ('MotionTemporalDenoise', dict(state_dtype=torch.float64), V, 'state_dtype must be float32 or float16, got torch.float64'),
    # ---- HdrMerge: range, pattern, even; radius, clip, thresholds, pixel_threshold, variance_floor, model
    *_size_rows('HdrMerge', MOSAIC_EVEN, pattern_first=True),
    *_window_rows('HdrMerge'),
    ('HdrMerge', dict(clip=0), V, 'clip must be finite and > 0, got 0'),
    ('HdrMerge', dict(clip=1e-50), V, 'clip must be finite and > 0, got 1e-50'),   # (the caller's value, not the rounded one)
    ('HdrMerge', dict(clip=1e39), V, 'clip must be finite and > 0, got 1e+39'),
    ('HdrMerge', dict(clip=NAN), V, 'clip must be finite and > 0, got nan'),
    ('HdrMerge', dict(radius=1, clip=0), V, RADIUS_MSG.format(1)),
    ('HdrMerge', dict(clip=-1, thresholds=(1,)), V, 'clip must be finite and > 0, got -1'),
    ('HdrMerge', dict(pixel_threshold=0, variance_floor=0), V, 'pixel_threshold must be finite and > 0, or None, got 0'),
    # ---- MotionHdrMerge: the base first, then motion
    *_size_rows('MotionHdrMerge', MOSAIC_EVEN, pattern_first=True),
    *_window_rows('MotionHdrMerge'),
    ('MotionHdrMerge', dict(clip=0), V, 'clip must be finite and > 0, got 0'),
    ('MotionHdrMerge', dict(motion='x'), T, 'motion must be a MotionEstimate, got str'),
    ('MotionHdrMerge', dict(motion=New('MotionEstimate', image_size=(32, 8))), V, 'motion is for (32, 8), the merge for (16, 8)'),
    ('MotionHdrMerge', dict(radius=1, motion='x'), V, RADIUS_MSG.format(1)),
    ('MotionHdrMerge', dict(noise_model=None, motion='x'), T, 'noise_model must be a NoiseModel, got NoneType'),
    ('MotionHdrMerge', dict(device=CPU, motion='x'), V, DEVICE_MSG),
    # ---- MotionEstimate: range, even (no pattern); levels, search, zero_bias, white_level
    *_size_rows('MotionEstimate', MOSAIC_EVEN, pattern_first=False, pattern=False),
    ('MotionEstimate', dict(levels=0), V, 'levels must be an integer in 1..4, got 0'),
    ('MotionEstimate', dict(levels=5), V, 'levels must be an integer in 1..4, got 5'),
    ('MotionEstimate', dict(levels=True), V, 'levels must be an integer in 1..4, got True'),
    ('MotionEstimate', dict(levels=1.5), V, 'levels must be an integer in 1..4, got 1.5'),
    ('MotionEstimate', dict(search=0), V, 'search must be an integer in 1..4, got 0'),
    ('MotionEstimate', dict(search=5), V, 'search must be an integer in 1..4, got 5'),
    ('MotionEstimate', dict(zero_bias=-1), V, 'zero_bias must be an integer in 0..65535, got -1'),
    ('MotionEstimate', dict(zero_bias=65536), V, 'zero_bias must be an integer in 0..65535, got 65536'),
    ('MotionEstimate', dict(zero_bias=1.0), V, 'zero_bias must be an integer in 0..65535, got 1.0'),
    ('MotionEstimate', dict(zero_bias=False), V, 'zero_bias must be an integer in 0..65535, got False'),
    ('MotionEstimate', dict(white_level=0), V, 'white_level must be finite and > 0 with a finite 1 / (4 white_level), got 0'),
    ('MotionEstimate', dict(white_level=INF), V, 'white_level must be finite and > 0 with a finite 1 / (4 white_level), got inf'),
    ('MotionEstimate', dict(white_level=1e-45), V, 'white_level must be finite and > 0 with a finite 1 / (4 white_level), got 1e-45'),
    ('MotionEstimate', dict(image_size=(16, 7), levels=0), V, MOSAIC_EVEN.format('16x7')),
    ('MotionEstimate', dict(levels=0, search=0), V, 'levels must be an integer in 1..4, got 0'),
    ('MotionEstimate', dict(search=0, zero_bias=-1), V, 'search must be an integer in 1..4, got 0'),
    ('MotionEstimate', dict(zero_bias=-1, white_level=0), V, 'zero_bias must be an integer in 0..65535, got -1'),
    # ---- Highlights: range, even, pattern; mode, threshold, low, min_count
    *_size_rows('Highlights', IMAGE_EVEN, pattern_first=False),
    ('Highlights', dict(mode='x'), V, "mode must be 'opposed' or 'clip', got 'x'"),
    ('Highlights', dict(bayer_pattern=None, mode='x'), V, 'Invalid bayer pattern: None'),
    ('Highlights', dict(threshold=0), V, 'threshold must lie in (0, 1], got 0'),
    ('Highlights', dict(threshold=1.5), V, 'threshold must lie in (0, 1], got 1.5'),
    ('Highlights', dict(mode='x', threshold=0), V, "mode must be 'opposed' or 'clip', got 'x'"),
    ('Highlights', dict(low=1.0), V, 'low must lie in [0, 1), got 1.0'),
    ('Highlights', dict(low=-0.1), V, 'low must lie in [0, 1), got -0.1'),
    ('Highlights', dict(threshold=NAN, low=1), V, 'threshold must lie in (0, 1], got nan'),
    ('Highlights', dict(min_count=0), V, 'min_count must be an integer >= 1, got 0'),
    ('Highlights', dict(min_count=1.5), V, 'min_count must be an integer >= 1, got 1.5'),
    ('Highlights', dict(min_count=2 ** 31), V, 'min_count must be an integer >= 1, got 2147483648'),
    ('Highlights', dict(low=1, min_count=0), V, 'low must lie in [0, 1), got 1'),
    # ---- RawPrepare: range, even, pattern; black and white, threshold, ratio, min_count, shading
    *_size_rows('RawPrepare', IMAGE_EVEN, pattern_first=False),
    ('RawPrepare', dict(black=(1, 2, 3)), V, 'black must be one level or four (one per CFA position), got 3'),
    ('RawPrepare', dict(bayer_pattern=None, black=(1, 2, 3)), V, 'Invalid bayer pattern: None'),
    ('RawPrepare', dict(black=NAN), V, 'black and white must be finite'),
    ('RawPrepare', dict(white=INF), V, 'black and white must be finite'),
    ('RawPrepare', dict(white=0), V, 'white (0) must lie above every black level ([0.0, 0.0, 0.0, 0.0])'),
    ('RawPrepare', dict(black=(1, 2, 3, 4096.5)), V, 'white (4095.0) must lie above every black level ([1.0, 2.0, 3.0, 4096.5])'),
    ('RawPrepare', dict(black=-1e39), V, 'black and 1 / (white - black) must be finite in float32'),
    ('RawPrepare', dict(white=0, threshold=-1), V, 'white (0) must lie above every black level ([0.0, 0.0, 0.0, 0.0])'),
    ('RawPrepare', dict(threshold=-1), V, 'threshold must be finite and >= 0, got -1'),
    ('RawPrepare', dict(threshold=INF), V, 'threshold must be finite and >= 0, got inf'),
    ('RawPrepare', dict(ratio=0), V, 'ratio must lie in (0, 1], got 0'),
    ('RawPrepare', dict(ratio=1.5), V, 'ratio must lie in (0, 1], got 1.5'),
    ('RawPrepare', dict(threshold=-1, ratio=0), V, 'threshold must be finite and >= 0, got -1'),
    ('RawPrepare', dict(min_count=0), V, 'min_count must be 1..4, got 0'),
    ('RawPrepare', dict(min_count=5), V, 'min_count must be 1..4, got 5'),
    ('RawPrepare', dict(min_count=2.5), V, 'min_count must be 1..4, got 2.5'),
    ('RawPrepare', dict(ratio=2, min_count=5), V, 'ratio must lie in (0, 1], got 2'),
    ('RawPrepare', dict(shading=z(2, 2, 3)), V, 'shading must be (grid_height, grid_width, 4), got (2, 2, 3)'),
    ('RawPrepare', dict(shading=z(2, 2)), V, 'shading must be (grid_height, grid_width, 4), got (2, 2)'),
    ('RawPrepare', dict(shading=z(2, 1, 4)), V, 'shading grid must be 2..257 nodes per axis, got 1x2'),
    ('RawPrepare', dict(shading=z(258, 2, 4)), V, 'shading grid must be 2..257 nodes per axis, got 2x258'),
    ('RawPrepare', dict(shading=z(2, 5, 4)), V, 'shading grid 5x2 too dense for a 16x8 frame (nodes must be at least 4 pixels apart)'),
    ('RawPrepare', dict(shading=z(3, 2, 4)), V, 'shading grid 2x3 too dense for a 16x8 frame (nodes must be at least 4 pixels apart)'),
    ('RawPrepare', dict(min_count=5, shading=z(2, 2)), V, 'min_count must be 1..4, got 5'),
    # ---- ChromaticAberration: range, pattern, even; interp, center, rn, model
    *_size_rows('ChromaticAberration', MOSAIC_EVEN, pattern_first=True),
    ('ChromaticAberration', dict(interp='x'), V, "interp must be 'bilinear' or 'bicubic', got 'x'"),
    ('ChromaticAberration', dict(image_size=(16, 7), interp='x'), V, MOSAIC_EVEN.format('16x7')),
    ('ChromaticAberration', dict(center=(1, 2, 3)), V, 'center must be (x0, y0), got (1, 2, 3)'),
    ('ChromaticAberration', dict(center=(NAN, 0)), V, 'center must be finite, got (nan, 0)'),
    ('ChromaticAberration', dict(center=[1e39, 0]), V, 'center must be finite, got (1e+39, 0)'),
    ('ChromaticAberration', dict(interp='x', center=(1,)), V, "interp must be 'bilinear' or 'bicubic', got 'x'"),
    ('ChromaticAberration', dict(rn=0), V, 'rn must be finite and > 0, got 0.0'),      # (the rounded value)
    ('ChromaticAberration', dict(rn=1e-50), V, 'rn must be finite and > 0, got 0.0'),
    ('ChromaticAberration', dict(rn=1e39), V, 'rn must be finite and > 0, got inf'),
    ('ChromaticAberration', dict(center=(1,), rn=0), V, 'center must be (x0, y0), got (1,)'),
    ('ChromaticAberration', dict(model=z(3, 4)), V, 'model must be a contiguous (2, 4) float32 tensor, got (3, 4) torch.float32'),
    ('ChromaticAberration', dict(model=z(2, 4, dtype=torch.float64)), V, 'model must be a contiguous (2, 4) float32 tensor, got (2, 4) torch.float64'),
    ('ChromaticAberration', dict(model=z(2, 8)[:, ::2]), V, 'model must be a contiguous (2, 4) float32 tensor, got (2, 4) torch.float32'),
    ('ChromaticAberration', dict(model='x'), V, 'model must be a contiguous (2, 4) float32 tensor, got () str'),
    ('ChromaticAberration', dict(rn=-1, model='x'), V, 'rn must be finite and > 0, got -1.0'),
    ('ChromaticAberration.from_coefficients', dict(red=(1, 2)), V, 'red must be three finite values (v, c, b), got (1.0, 2.0)'),
    ('ChromaticAberration.from_coefficients', dict(blue=(1, NAN, 0)), V, 'blue must be three finite values (v, c, b), got (1.0, nan, 0.0)'),
    ('ChromaticAberration.from_coefficients', dict(red=(1,), blue=(1,)), V, 'red must be three finite values (v, c, b), got (1.0,)'),
    ('ChromaticAberration.from_coefficients', dict(device=CPU, blue=(1,)), V, 'blue must be three finite values (v, c, b), got (1.0,)'),
    ('ChromaticAberration.from_coefficients', dict(device=CPU), V, DEVICE_MSG),
    ('ChromaticAberration.from_coefficients', dict(image_size=(15, 8)), V, MOSAIC_EVEN.format('15x8')),
    # ---- NoiseProfile: range, pattern, even; bins, white, clip, min_count, max_frames
    *_size_rows('NoiseProfile', MOSAIC_EVEN, pattern_first=True),
    ('NoiseProfile', dict(bins=1), V, 'bins must be an integer in 2..32, got 1'),
    ('NoiseProfile', dict(bins=33), V, 'bins must be an integer in 2..32, got 33'),
    ('NoiseProfile', dict(bins=2.5), V, 'bins must be an integer in 2..32, got 2.5'),
    ('NoiseProfile', dict(image_size=(16, 7), bins=1), V, MOSAIC_EVEN.format('16x7')),
    ('NoiseProfile', dict(white=0), V, 'white must be finite and > 0, got 0.0'),
    ('NoiseProfile', dict(white=1e-45), V, 'white must be finite and > 0, got 1.401298464324817e-45'),
    ('NoiseProfile', dict(white=INF), V, 'white must be finite and > 0, got inf'),
    ('NoiseProfile', dict(bins=1, white=0), V, 'bins must be an integer in 2..32, got 1'),
    ('NoiseProfile', dict(clip=(1, 2, 3)), V, 'clip must be integers (clip_lo, clip_hi) with 0 <= clip_lo <= clip_hi <= 65535, got (1, 2, 3)'),
    ('NoiseProfile', dict(clip=(5, 1)), V, 'clip must be integers (clip_lo, clip_hi) with 0 <= clip_lo <= clip_hi <= 65535, got (5, 1)'),
    ('NoiseProfile', dict(clip=[0.5, 1]), V, 'clip must be integers (clip_lo, clip_hi) with 0 <= clip_lo <= clip_hi <= 65535, got (0.5, 1)'),
    ('NoiseProfile', dict(clip=(0, 65536)), V, 'clip must be integers (clip_lo, clip_hi) with 0 <= clip_lo <= clip_hi <= 65535, got (0, 65536)'),
    ('NoiseProfile', dict(white=-1, clip=(5, 1)), V, 'white must be finite and > 0, got -1.0'),
    ('NoiseProfile', dict(min_count=0), V, 'min_count must be an integer >= 1, got 0'),
    ('NoiseProfile', dict(clip=(5, 1), min_count=0), V, 'clip must be integers (clip_lo, clip_hi) with 0 <= clip_lo <= clip_hi <= 65535, got (5, 1)'),
    ('NoiseProfile', dict(max_frames=0), V, 'max_frames must be an integer in 1..16, got 0'),
    ('NoiseProfile', dict(max_frames=17), V, 'max_frames must be an integer in 1..16, got 17'),
    ('NoiseProfile', dict(min_count=1.5, max_frames=0), V, 'min_count must be an integer >= 1, got 1.5'),
    ('NoiseModel', dict(model=z(2, 4)), V, 'model must be a contiguous (3, 4) float32 tensor, got (2, 4) torch.float32'),
    # ---- FrameStats: its own range; pattern, even and channels only in the mosaic mode
    ('FrameStats', dict(device=CPU), V, DEVICE_MSG),
    ('FrameStats', dict(image_size=(0, 8)), V, 'Image dimensions must be 1..65535, got 0x8'),
    ('FrameStats', dict(image_size=(16, 65536)), V, 'Image dimensions must be 1..65535, got 16x65536'),
    ('FrameStats', dict(image_size=(0, 8), bayer_pattern='RGGB'), V, 'Image dimensions must be 1..65535, got 0x8'),
    ('FrameStats', dict(bayer_pattern='RGGB'), V, PATTERN_MSG),
    ('FrameStats', dict(image_size=(15, 8), bayer_pattern='RGGB'), V, PATTERN_MSG),
    ('FrameStats', dict(image_size=(15, 8), bayer_pattern=PATTERN), V, MOSAIC_EVEN.format('15x8')),
    ('FrameStats', dict(image_size=(1, 8), bayer_pattern=PATTERN), V, MOSAIC_EVEN.format('1x8')),
    ('FrameStats', dict(image_size=(16, 7), bayer_pattern=PATTERN, channels=1), V, MOSAIC_EVEN.format('16x7')),
    ('FrameStats', dict(bayer_pattern=PATTERN, channels=1), V, 'a mosaic has channels = 3 (R, G, B), got 1'),
    ('FrameStats', dict(channels=2), V, 'channels must be 1 or 3, got 2'),
    ('FrameStats', dict(image_size=(0, 8), channels=2), V, 'Image dimensions must be 1..65535, got 0x8'),
    ('FrameStats', dict(channels=2, bins=1), V, 'channels must be 1 or 3, got 2'),
    ('FrameStats', dict(bins=1), V, 'bins must be an integer in 2..1024, got 1'),
    ('FrameStats', dict(value_range=(1, 2, 3)), V, 'value_range must be (lo, hi), got (1, 2, 3)'),
    ('FrameStats', dict(value_range=(1.0, 0.0)), V, 'value_range must be finite with lo < hi, got (1.0, 0.0)'),
    ('FrameStats', dict(stride=0), V, 'stride must be an integer in 1..65535, got 0'),
    ('FrameStats', dict(quantiles=(0.5, 1.5)), V, 'quantiles must be at most 8 fractions in [0, 1], got (0.5, 1.5)'),
    ('FrameStats', dict(max_frames=17), V, 'max_frames must be an integer in 1..16, got 17'),
    ('FrameStats', dict(min_count=0), V, 'min_count must be an integer >= 1, got 0'),
    # ---- ImageProcessor: the slots of the mosaic stages, refused before anything else of the processor is made
    ('ImageProcessor', dict(raw_correction=New('RawPrepare', image_size=(32, 8))), V, 'raw_correction is for (32, 8) RGGB, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(raw_correction=New('RawPrepare', bayer_pattern=New('BayerPattern.BGGR'))), V,
     'raw_correction is for (16, 8) BGGR, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(image_size=[16, 8], raw_correction=New('RawPrepare', image_size=(32, 8)), temporal='x'), V,
     'raw_correction is for (32, 8) RGGB, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(temporal='x'), T, 'temporal must be a TemporalDenoise or None, got str (pass the arguments behind storage_dtype by keyword)'),
    ('ImageProcessor', dict(temporal=New('MotionTemporalDenoise', image_size=(32, 8))), V, 'temporal is for (32, 8) RGGB, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(temporal=New('TemporalDenoise', bayer_pattern=New('BayerPattern.GRBG')), hdr='x'), V,
     'temporal is for (16, 8) GRBG, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(hdr=torch.float32), T, 'hdr must be an HdrMerge or None, got dtype (pass the arguments behind padding by keyword)'),
    ('ImageProcessor', dict(hdr=New('MotionHdrMerge', image_size=(16, 16))), V, 'hdr is for (16, 16) RGGB, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(hdr=New('HdrMerge', bayer_pattern=New('BayerPattern.GBRG')), chromatic=0), V, 'hdr is for (16, 8) GBRG, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(chromatic=0), T, 'chromatic must be a ChromaticAberration or None, got int (pass it and padding by keyword)'),
    ('ImageProcessor', dict(chromatic=New('ChromaticAberration', image_size=(8, 16))), V, 'chromatic is for (8, 16) RGGB, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(chromatic=New('ChromaticAberration', bayer_pattern=New('BayerPattern.BGGR')), highlights='x'), V,
     'chromatic is for (16, 8) BGGR, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(highlights='x'), T, 'highlights must be a Highlights or None, got str (color is the argument after it: pass both by keyword)'),
    ('ImageProcessor', dict(highlights=New('Highlights', image_size=(32, 8))), V, 'highlights is for (32, 8) RGGB, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(highlights=New('Highlights', bayer_pattern=New('BayerPattern.BGGR')), white_balance=(1, 1, 1)), V,
     'highlights is for (16, 8) BGGR, the processor for (16, 8) RGGB'),
    ('ImageProcessor', dict(highlights=New('Highlights')), V, 'highlights needs white_balance: it applies the gains itself'),
    ('ImageProcessor', dict(exposure=New('FrameStats', image_size=(32, 8))), V, 'exposure is for 32x8, the processor for 16x8'),
    ('ImageProcessor', dict(exposure=New('FrameStats', bayer_pattern=PATTERN)), V, 'exposure measures the demosaiced frames: it needs channels=3 and no bayer_pattern'),
]

_ME = 'MotionEstimate(16x8, levels=3, search=4, zero_bias={}, white_level=1)'
REPRS = [
    ('TemporalDenoise', {}, 'TemporalDenoise(16x8, RGGB, radius=2, thresholds=(1.5, 3), pixel_threshold=4, max_frames=8, state_dtype=torch.float32)'),
    ('TemporalDenoise', dict(image_size=(65534, 2), bayer_pattern=New('BayerPattern.GBRG'), radius=3.0, thresholds=[0.1, 2.5], pixel_threshold=None, max_frames=1,
                             variance_floor=1e-6, state_dtype=torch.float16),
     'TemporalDenoise(65534x2, GBRG, radius=3, thresholds=(0.1, 2.5), pixel_threshold=None, max_frames=1, state_dtype=torch.float16)'),
    ('MotionTemporalDenoise', {}, 'MotionTemporalDenoise(16x8, RGGB, radius=2, thresholds=(1.5, 3), pixel_threshold=4, max_frames=8, state_dtype=torch.float32, '
                                  'motion=' + _ME.format(300) + ')'),
    ('MotionTemporalDenoise', dict(pixel_threshold=0.1, max_frames=2.5, motion=New('MotionEstimate', levels=1, search=2, zero_bias=0, white_level=0.5)),
     'MotionTemporalDenoise(16x8, RGGB, radius=2, thresholds=(1.5, 3), pixel_threshold=0.1, max_frames=2.5, state_dtype=torch.float32, '
     'motion=MotionEstimate(16x8, levels=1, search=2, zero_bias=0, white_level=0.5))'),
    ('HdrMerge', {}, 'HdrMerge(16x8, RGGB, radius=2, clip=0.95, thresholds=(1.5, 3), pixel_threshold=4)'),
    ('HdrMerge', dict(image_size=(2, 65534), bayer_pattern=New('BayerPattern.BGGR'), radius=3, clip=0.5, thresholds=(1, 2), pixel_threshold=None),
     'HdrMerge(2x65534, BGGR, radius=3, clip=0.5, thresholds=(1, 2), pixel_threshold=None)'),
    ('MotionHdrMerge', {}, 'MotionHdrMerge(16x8, RGGB, radius=2, clip=0.95, thresholds=(1.5, 3), pixel_threshold=4, motion=' + _ME.format(750) + ')'),
    ('MotionHdrMerge', dict(clip=2, pixel_threshold=1e-3, motion=New('MotionEstimate')),
     'MotionHdrMerge(16x8, RGGB, radius=2, clip=2, thresholds=(1.5, 3), pixel_threshold=0.001, motion=' + _ME.format(300) + ')'),
    ('MotionEstimate', {}, _ME.format(300)),
    ('MotionEstimate', dict(image_size=(64, 34), levels=4, search=1, zero_bias=65535, white_level=4095),
     'MotionEstimate(64x34, levels=4, search=1, zero_bias=65535, white_level=4095)'),
    ('Highlights', {}, 'Highlights(16x8, RGGB, mode=opposed, threshold=0.98, low=0.2, min_count=64)'),
    ('Highlights', dict(bayer_pattern=New('BayerPattern.GRBG'), mode='clip', threshold=1, low=0, min_count=1),
     'Highlights(16x8, GRBG, mode=clip, threshold=1, low=0, min_count=1)'),
    ('RawPrepare', {}, 'RawPrepare(16x8, RGGB, black=[0.0, 0.0, 0.0, 0.0], white=4095, clip=True)'),
    ('RawPrepare', dict(black=(1, 2, 3, 4), white=1023, hot=True, dead=True, threshold=0.5, ratio=1, min_count=4, clip=False),
     'RawPrepare(16x8, RGGB, black=[1.0, 2.0, 3.0, 4.0], white=1023, defects=hot+dead(threshold=0.5, ratio=1, min_count=4), clip=False)'),
    ('ChromaticAberration', {}, 'ChromaticAberration(16x8, RGGB, center=(7.5, 3.5), rn=8.27647, interp=bilinear)'),
    ('ChromaticAberration', dict(center=(1, 2), rn=10, interp='bicubic', model=z(2, 4)), 'ChromaticAberration(16x8, RGGB, center=(1, 2), rn=10, interp=bicubic)'),
    ('NoiseProfile', {}, 'NoiseProfile(16x8, RGGB, bins=32, white=1, clip=(1, 64224), min_count=32, max_frames=1)'),
    ('NoiseProfile', dict(bins=2, white=65535, clip=[0, 65535], min_count=1, max_frames=16),
     'NoiseProfile(16x8, RGGB, bins=2, white=65535, clip=(0, 65535), min_count=1, max_frames=16)'),
    ('FrameStats', {}, 'FrameStats(16x8, 3 channels, bins=256, range=(0, 1), stride=1, quantiles=(0.001, 0.5, 0.999), max_frames=1, min_count=64)'),
    ('FrameStats', dict(image_size=(1, 3), channels=1, bins=2, quantiles=()),
     'FrameStats(1x3, 1 channel, bins=2, range=(0, 1), stride=1, quantiles=(), max_frames=1, min_count=64)'),
    ('FrameStats', dict(bayer_pattern=PATTERN, stride=4, max_frames=6),
     'FrameStats(16x8, RGGB, bins=256, range=(0, 1), stride=4, quantiles=(0.001, 0.5, 0.999), max_frames=6, min_count=64)'),
]

_BRACKET = 'HdrMerge input shape {} of frame {} != expected (8, 16)'   # (the literal class name, also of MotionHdrMerge)
_REF_MSG = 'ref must be None or a frame index below 2, got {}'


def _temporal_calls(cls):
    return [(cls, {}, 'process', (SMALL,), {}, R, f'{cls} input shape (8, 8) != expected (8, 16)'),
            (cls, {}, 'process', (z(8, 16, 1),), {}, R, f'{cls} input shape (8, 16, 1) != expected (8, 16)'),
            (cls, {}, 'process', (SMALL,), dict(out_dtype=torch.float64), R, f'{cls} input shape (8, 8) != expected (8, 16)'),
            (cls, {}, 'process', (FRAME,), dict(out_dtype=torch.float64), V, OUT_DTYPE_MSG),
            (cls, {}, 'process', (z(8, 16, dtype=torch.float64),), {}, V, OUT_DTYPE_MSG),   # (out_dtype None is the input's)
            (cls, {}, 'process', (FRAME,), dict(gains='x'), R, CUDA_MSG),
            (cls, {}, 'process', (HALF,), dict(key='left', out_dtype=torch.float32), R, CUDA_MSG),
            (cls, {}, 'reset', ('left',), {}, K, "TemporalDenoise has no state for key 'left'")]


def _bracket_calls(cls):
    """HdrMerge.process and, with the same checks, MotionHdrMerge.process and .align."""
    pair, e = [FRAME, FRAME], (1.0, 0.25)
    return [(cls, {}, 'process', (FRAME, e), {}, R, 'HdrMerge input shape (8, 16): a stacked bracket is (F, H, W)'),
            (cls, {}, 'process', (z(1, 8, 16), e), {}, V, 'a bracket has 2..8 frames, got 1'),
            (cls, {}, 'process', ([FRAME] * 9, e), {}, V, 'a bracket has 2..8 frames, got 9'),
            (cls, {}, 'process', ([], e), {}, V, 'a bracket has 2..8 frames, got 0'),
            (cls, {}, 'process', ([FRAME, SMALL], e), {}, R, _BRACKET.format('(8, 8)', 1)),
            (cls, {}, 'process', (z(2, 8, 8), e), {}, R, _BRACKET.format('(8, 8)', 0)),
            (cls, {}, 'process', ([FRAME, None], e), {}, R, _BRACKET.format('()', 1)),
            (cls, {}, 'process', ([FRAME, SMALL], e), dict(out_dtype=torch.float64, ref=5), R, _BRACKET.format('(8, 8)', 1)),
            (cls, {}, 'process', (pair, e), dict(out_dtype=torch.float64, ref=5), V, OUT_DTYPE_MSG),
            (cls, {}, 'process', ([z(8, 16, dtype=torch.int32)] * 2, e), {}, V, 'out_dtype must be float32 or float16, got torch.int32'),
            (cls, {}, 'process', (pair, e), dict(ref=2), V, _REF_MSG.format(2)),
            (cls, {}, 'process', (pair, e), dict(ref=-1), V, _REF_MSG.format(-1)),
            (cls, {}, 'process', (pair, e), dict(ref=True), V, _REF_MSG.format(True)),
            (cls, {}, 'process', (pair, e), dict(ref=0.5), V, _REF_MSG.format(0.5)),
            (cls, {}, 'process', (pair, (1.0,)), dict(ref=2), V, _REF_MSG.format(2)),
            (cls, {}, 'process', (pair, (1.0, 0.5, 0.25)), dict(ref=0), V, '2 frames need 2 exposures, got 3'),
            (cls, {}, 'process', (pair, (1.0, 0.0)), dict(ref=0), V, 'exposures must be finite and > 0 as float32, got (1.0, 0.0)'),
            (cls, {}, 'process', (pair, [1, 1e-50]), dict(ref=0), V, 'exposures must be finite and > 0 as float32, got (1, 1e-50)'),
            (cls, {}, 'process', (pair, (1.0, INF)), dict(ref=1), V, 'exposures must be finite and > 0 as float32, got (1.0, inf)'),
            (cls, {}, 'process', (pair, z(3)), dict(ref=0), R, 'exposures must be a contiguous (2,) float32 tensor'),
            (cls, {}, 'process', (pair, z(2, dtype=torch.float64)), dict(ref=0), R, 'exposures must be a contiguous (2,) float32 tensor'),
            (cls, {}, 'process', (pair, z(4)[::2]), dict(ref=0), R, 'exposures must be a contiguous (2,) float32 tensor'),
            (cls, {}, 'process', (pair, e), {}, R, CUDA_MSG),
            (cls, {}, 'process', (z(2, 8, 16, dtype=torch.float16), z(2)), dict(ref=1, return_mask=True), R, CUDA_MSG)]


CALLS = [
    *_temporal_calls('TemporalDenoise'),
    *_temporal_calls('MotionTemporalDenoise'),
    *_bracket_calls('HdrMerge'),
    *_bracket_calls('MotionHdrMerge'),
    *[(c, k, 'align', a[:2], {n: v for n, v in kw.items() if n == 'ref'}, x, m) for c, k, _, a, kw, x, m in _bracket_calls('MotionHdrMerge') if 'out_dtype' not in kw],
    ('MotionHdrMerge', {}, 'process', ([FRAME, SMALL], z(2)), {}, V, 'ref=None needs exposures the host holds: with a device tensor of exposures pass the anchor frame as ref'),
    ('MotionHdrMerge', {}, 'align', ([FRAME, SMALL], z(2)), {}, V, 'ref=None needs exposures the host holds: with a device tensor of exposures pass the anchor frame as ref'),
    ('MotionHdrMerge', {}, 'process', ([FRAME, FRAME], (1.0, 0.25)), dict(fields=z(2, 1, 1, 2)), R, 'fields must be a contiguous (2, 1, 1, 2) int16 tensor'),
    ('MotionHdrMerge', {}, 'process', ([FRAME] * 3, (1.0, 0.25)), dict(fields=z(2, 1, 1, 2, dtype=torch.int16), ref=7), R,
     'fields must be a contiguous (3, 1, 1, 2) int16 tensor'),
    ('MotionHdrMerge', dict(image_size=(66, 34)), 'process', (z(2, 34, 66), (1.0, 0.25)), dict(fields='x', out_dtype=torch.float64), R,
     'fields must be a contiguous (2, 2, 2, 2) int16 tensor'),
    ('MotionHdrMerge', {}, 'process', ([FRAME, SMALL], (1.0, 0.25)), dict(fields='x'), R, _BRACKET.format('(8, 8)', 1)),
    ('MotionHdrMerge', {}, 'process', ([FRAME, FRAME], (1.0, 0.25)), dict(fields=z(2, 1, 1, 2, dtype=torch.int16), ref=2), V, _REF_MSG.format(2)),
    ('MotionHdrMerge', {}, 'process', ([FRAME, FRAME], (1.0, 0.25)), dict(fields=z(2, 1, 1, 2, dtype=torch.int16)), R, CUDA_MSG),
    ('MotionHdrMerge', {}, 'prepare', (1,), {}, V, 'a bracket has 2..8 frames, got 1'),
    ('MotionHdrMerge', {}, 'prepare', (9,), {}, V, 'a bracket has 2..8 frames, got 9'),
    ('MotionHdrMerge', {}, 'prepare', (2.5,), {}, V, 'a bracket has 2..8 frames, got 2.5'),
    ('MotionHdrMerge', {}, 'prepare', (True,), {}, V, 'a bracket has 2..8 frames, got True'),
    ('MotionHdrMerge', {}, 'fields', (), {}, R, 'MotionHdrMerge: no bracket has been aligned yet (prepare, align or process come first)'),
    ('MotionHdrMerge', {}, 'costs', (), {}, R, 'MotionHdrMerge: no bracket has been aligned yet (prepare, align or process come first)'),
    # ---- MotionEstimate
    ('MotionEstimate', {}, 'estimate', (SMALL, FRAME), {}, R, 'MotionEstimate cur shape (8, 8) != expected (8, 16)'),
    ('MotionEstimate', {}, 'estimate', (SMALL, SMALL), {}, R, 'MotionEstimate cur shape (8, 8) != expected (8, 16)'),
    ('MotionEstimate', {}, 'estimate', (FRAME, SMALL), {}, R, CUDA_MSG),   # (all of cur is looked at before ref)
    ('MotionEstimate', {}, 'estimate', (FRAME, FRAME), dict(return_costs=True), R, CUDA_MSG),
    ('MotionEstimate', {}, 'build_pyramid', (z(16, 8), None, 0), {}, R, 'MotionEstimate input shape (16, 8) != expected (8, 16)'),
    ('MotionEstimate', {}, 'build_pyramid', (FRAME, None, 0), {}, R, CUDA_MSG),
    # ---- Highlights and RawPrepare: the dimension is an assertion
    ('Highlights', {}, 'process', (z(8, 16, 1), (1, 1, 1)), {}, A, 'mosaic must have 2 dimensions, got torch.Size([8, 16, 1])'),
    ('Highlights', {}, 'process', (SMALL, (1, 1, 1)), dict(out_dtype=torch.float64), R, 'Highlights input shape (8, 8) != expected (8, 16)'),
    ('Highlights', {}, 'process', (FRAME, 'x'), dict(out_dtype=torch.float64), R, CUDA_MSG),
    ('Highlights', {}, 'chrominance', (z(8),  (1, 1, 1)), {}, A, 'mosaic must have 2 dimensions, got torch.Size([8])'),
    ('Highlights', {}, 'chrominance', (SMALL, (1, 1, 1)), {}, R, 'Highlights input shape (8, 8) != expected (8, 16)'),
    ('Highlights', {}, 'chrominance', (FRAME, (1, 1, 1)), {}, R, CUDA_MSG),
    ('Highlights', {}, 'statistics', (SMALL, (1, 1, 1)), {}, R, 'Highlights input shape (8, 8) != expected (8, 16)'),
    ('Highlights', {}, 'statistics', (HALF, (1, 1, 1)), {}, R, CUDA_MSG),
    ('RawPrepare', {}, 'process', (z(8, 16, 1),), {}, A, 'mosaic must have 2 dimensions, got torch.Size([8, 16, 1])'),
    ('RawPrepare', {}, 'process', (SMALL,), dict(out_dtype=torch.float64), R, 'RawPrepare input shape (8, 8) != expected (8, 16)'),
    ('RawPrepare', {}, 'process', (z(8, 16, dtype=torch.int16),), dict(out_dtype=torch.float64, white_balance='x'), R, CUDA_MSG),
    ('RawPrepare', {}, 'process_packed', (z(192, dtype=torch.uint8),), dict(format_type=None), V, 'Unsupported packed format: None'),
    ('RawPrepare', {}, 'process_packed', (z(191, dtype=torch.uint8),), {}, R, CUDA_MSG),
    # ---- ChromaticAberration
    ('ChromaticAberration', {}, 'correct', (SMALL,), dict(out_dtype=torch.float64), R, 'ChromaticAberration input shape (8, 8) != expected (8, 16)'),
    ('ChromaticAberration', {}, 'correct', (None,), {}, R, 'ChromaticAberration input shape () != expected (8, 16)'),
    ('ChromaticAberration', {}, 'correct', (FRAME,), dict(out_dtype=torch.float64, model='x'), V, OUT_DTYPE_MSG),
    ('ChromaticAberration', {}, 'correct', (z(8, 16, dtype=torch.uint8),), {}, V, 'out_dtype must be float32 or float16, got torch.uint8'),
    ('ChromaticAberration', {}, 'correct', (FRAME,), dict(model='x'), R, CUDA_MSG),
    ('ChromaticAberration', {}, 'estimate', ([],), {}, V, 'estimate takes 1..16 frames, got 0'),
    ('ChromaticAberration', {}, 'estimate', ([FRAME] * 17,), {}, V, 'estimate takes 1..16 frames, got 17'),
    ('ChromaticAberration', {}, 'estimate', (z(17, 8, 16),), dict(fit='x'), V, 'estimate takes 1..16 frames, got 17'),
    ('ChromaticAberration', {}, 'estimate', (SMALL,), dict(noise_model='x'), R, 'ChromaticAberration input shape (8, 8) != expected (8, 16)'),
    ('ChromaticAberration', {}, 'estimate', ([FRAME, SMALL],), {}, R, 'ChromaticAberration input shape (8, 8) != expected (8, 16)'),
    ('ChromaticAberration', {}, 'estimate', ([FRAME, 1.0],), {}, R, 'ChromaticAberration input shape () != expected (8, 16)'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(noise_model='x', fit='x'), T, 'noise_model must be a NoiseModel or None, got str'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(fit='x', clip=0), V, "fit must be 'linear' or 'poly3', got 'x'"),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(clip=0, block=15), V, 'clip must be finite and > 0, got 0.0'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(clip=1e-50), V, 'clip must be finite and > 0, got 0.0'),   # (the rounded value, unlike HdrMerge)
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(clip=1e39), V, 'clip must be finite and > 0, got inf'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(block=15, max_shift=0), V, 'block must be an even integer in 16..256, got 15'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(block=17), V, 'block must be an even integer in 16..256, got 17'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(block=258), V, 'block must be an even integer in 16..256, got 258'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(block=True), V, 'block must be an even integer in 16..256, got True'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(max_shift=0), V, 'max_shift must be in (0, 8], got 0.0'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(max_shift=8.5), V, 'max_shift must be in (0, 8], got 8.5'),
    ('ChromaticAberration', {}, 'estimate', (FRAME,), dict(noise_model=MODEL), R, CUDA_MSG),
    ('ChromaticAberration', {}, 'estimate', ([HALF, HALF],), {}, R, CUDA_MSG),
    ('ChromaticAberration', {}, 'statistics', (SMALL,), {}, R, 'ChromaticAberration input shape (8, 8) != expected (8, 16)'),
    ('ChromaticAberration', {}, 'statistics', (FRAME,), dict(clip=-1), V, 'clip must be finite and > 0, got -1.0'),
    ('ChromaticAberration', {}, 'statistics', (FRAME,), dict(block=64), R, CUDA_MSG),
    ('ChromaticAberration', {}, 'refine', ([SMALL],), {}, R, 'ChromaticAberration input shape (8, 8) != expected (8, 16)'),
    ('ChromaticAberration', {}, 'with_model', (z(2, 3),), {}, V, 'model must be a contiguous (2, 4) float32 tensor, got (2, 3) torch.float32'),
    # ---- NoiseProfile, which words its own frame set, and the transform of its model
    ('NoiseProfile', {}, 'estimate', ([],), {}, V, 'NoiseProfile takes 1..1 frames per call (max_frames), got 0'),
    ('NoiseProfile', {}, 'estimate', ([FRAME, FRAME],), {}, V, 'NoiseProfile takes 1..1 frames per call (max_frames), got 2'),
    ('NoiseProfile', dict(max_frames=2), 'estimate', ([FRAME] * 3,), {}, V, 'NoiseProfile takes 1..2 frames per call (max_frames), got 3'),
    ('NoiseProfile', {}, 'estimate', (SMALL,), {}, R, 'NoiseProfile input shape (8, 8) != expected (8, 16)'),
    ('NoiseProfile', {}, 'statistics', (z(8, 16, 1),), {}, R, 'NoiseProfile input shape (8, 16, 1) != expected (8, 16)'),
    ('NoiseProfile', dict(max_frames=2), 'estimate', ([FRAME, SMALL],), {}, R, CUDA_MSG),   # (a frame is looked at whole before the next one)
    ('NoiseProfile', {}, 'estimate', (z(8, 16, dtype=torch.uint16),), {}, R, CUDA_MSG),
    ('NoiseModel', {}, 'stabilize', (FRAME,), dict(bayer_pattern='RGGB'), V, PATTERN_MSG),
    ('NoiseModel', {}, 'stabilize', (z(7, 16),), dict(bayer_pattern=PATTERN), V, 'stabilize: a mosaic is (H, W) with H and W even, 2..65535, got (7, 16)'),
    ('NoiseModel', {}, 'unstabilize', (z(8, 16, 1),), dict(bayer_pattern=PATTERN), V, 'unstabilize: a mosaic is (H, W) with H and W even, 2..65535, got (8, 16, 1)'),
    ('NoiseModel', {}, 'stabilize', (FRAME,), {}, V, 'stabilize: an image is (..., C) with C = 1 or 3, got (8, 16)'),
    ('NoiseModel', {}, 'stabilize', (z(0, 3),), {}, V, 'stabilize: empty input'),
    ('NoiseModel', {}, 'stabilize', (FRAME,), dict(bayer_pattern=PATTERN, sigma_out=0, out_dtype=torch.float64), V, 'sigma_out must be finite and > 0, got 0.0'),
    ('NoiseModel', {}, 'unstabilize', (FRAME,), dict(bayer_pattern=PATTERN, inverse='x', out_dtype=torch.float64), V, "inverse must be 'unbiased' or 'algebraic', got 'x'"),
    ('NoiseModel', {}, 'stabilize', (FRAME,), dict(bayer_pattern=PATTERN, out_dtype=torch.float64, gains='x'), V, OUT_DTYPE_MSG),
    ('NoiseModel', {}, 'unstabilize', (z(8, 16, dtype=torch.float64),), dict(bayer_pattern=PATTERN), V, OUT_DTYPE_MSG),
    ('NoiseModel', {}, 'stabilize', (z(4, 3),), dict(gains='x'), R, CUDA_MSG),
    ('NoiseModel', {}, 'unstabilize', (FRAME,), dict(bayer_pattern=PATTERN, gains='x'), R, CUDA_MSG),
    # ---- FrameStats in its mosaic mode
    ('FrameStats', dict(bayer_pattern=PATTERN), 'measure', ([],), {}, V, 'FrameStats takes 1..1 frames per call (max_frames), got 0'),
    ('FrameStats', dict(bayer_pattern=PATTERN), 'measure', (z(8, 16, 3),), {}, R, 'FrameStats input shape (8, 16, 3) != expected (8, 16)'),
    ('FrameStats', {}, 'measure', (FRAME,), {}, R, 'FrameStats input shape (8, 16) != expected (8, 16, 3)'),
    ('FrameStats', dict(bayer_pattern=PATTERN), 'white_balance', (FRAME,), {}, R, CUDA_MSG),
    ('FrameStats', dict(channels=1), 'white_balance', (FRAME,), {}, V, 'white_balance needs three channels'),
    ('FrameStats', dict(bayer_pattern=PATTERN, quantiles=()), 'bounds', (FRAME,), {}, V, 'bounds needs at least one quantile'),
]

ROWS = len(CONSTRUCT) + len(REPRS) + len(CALLS)
