"""CPU-only: the host layer of the stages on raw mosaics (torch_darktable/_mosaic.py) -- the stages derive from its base and take its
size, its frame filter and its workspace from it, an object built without a GPU holds no buffer, and the words of the shared checks
stand in the layer alone.  What the stages refuse, and in which words, is tests/test_mosaic_refusals.py."""

import re
from pathlib import Path

import pytest
import torch

PACKAGE = Path(__file__).resolve().parent.parent / 'torch-darktable_amd' / 'torch_darktable'
DEVICE = torch.device('cuda', 0)
SIZE = (16, 8)
# the modules of the stages on mosaics; RawCodec and LMMSE have limits and words of their own and are not part of the layer
MODULES = ('rawprepare', 'highlights', 'chromatic', 'noiseprofile', 'temporal', 'motion', 'hdrmerge', 'hdralign', 'framestats')


@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)   # (what the constructors ask; true of the machines without a GPU)


def stages(td):
    p, model = td.BayerPattern.RGGB, td.NoiseModel(torch.zeros(3, 4))
    return (td.RawPrepare(DEVICE, SIZE, p), td.Highlights(DEVICE, SIZE, p), td.ChromaticAberration(DEVICE, SIZE, p), td.NoiseProfile(DEVICE, SIZE, p),
            td.TemporalDenoise(DEVICE, SIZE, p, model), td.MotionEstimate(DEVICE, SIZE), td.MotionTemporalDenoise(DEVICE, SIZE, p, model),
            td.HdrMerge(DEVICE, SIZE, p, model), td.MotionHdrMerge(DEVICE, SIZE, p, model), td.FrameStats(DEVICE, SIZE, bayer_pattern=p), td.FrameStats(DEVICE, (5, 3)))


def test_the_stages_share_the_base(td, no_gpu):
    from torch_darktable._mosaic import MosaicStage

    for stage in stages(td):
        cls = type(stage)
        assert isinstance(stage, MosaicStage) and cls.__mro__[-2] is MosaicStage
        assert stage.image_size == (stage.width, stage.height) and stage._home_device() == DEVICE == stage._device
        assert cls.image_size is MosaicStage.image_size and cls._check_mosaic is MosaicStage._check_mosaic and cls._home_device is MosaicStage._home_device
        assert not hasattr(stage, '_cuda_device')
    assert td.MotionTemporalDenoise.__mro__[1] is td.TemporalDenoise and td.MotionHdrMerge.__mro__[1] is td.HdrMerge
    for cls in (td.Highlights, td.NoiseProfile, td.FrameStats):   # a workspace of a size fixed at construction: the base keeps it
        assert cls._workspace is MosaicStage._workspace
    for cls in (td.RawCodec, td.LMMSE, td.NoiseModel, td.Sharpen, td.Dehaze):
        assert not issubclass(cls, MosaicStage)
    assert td.TemporalDenoise.noise_model is td.HdrMerge.noise_model and isinstance(td.HdrMerge.noise_model, property)
    assert td.MotionTemporalDenoise.process is not td.TemporalDenoise.process and td.MotionTemporalDenoise._begin is td.TemporalDenoise._begin


def test_the_base_alone(td):
    from torch_darktable import _mosaic

    base = _mosaic.MosaicStage(DEVICE, [4.0, 6])
    assert base.image_size == (4, 6) and isinstance(base.width, int)
    assert _mosaic.MosaicStage(DEVICE, (1, 65535), min_size=1).image_size == (1, 65535)
    with pytest.raises(ValueError, match=r'^Device must be CUDA, got cpu$'):
        _mosaic.MosaicStage(torch.device('cpu'), (0, 6))
    with pytest.raises(ValueError, match=r'^Image dimensions must be 2\.\.65535, got 1x6$'):
        _mosaic.MosaicStage(DEVICE, (1, 6))
    with pytest.raises(ValueError, match=r'^Image dimensions must be 1\.\.65535, got 0x6$'):
        _mosaic.MosaicStage(DEVICE, (0, 6), min_size=1)
    _mosaic.MosaicStage(DEVICE, (4, 6))._check_even()
    with pytest.raises(ValueError, match=r'^Frame dimensions must be even \(whole CFA cells\), got 5x6$'):
        _mosaic.MosaicStage(DEVICE, (5, 6))._check_even('Frame')
    with pytest.raises(RuntimeError, match=r'^MosaicStage bracket shape \(6, 5\) != expected \(6, 4\)$'):
        base._check_mosaic(torch.zeros(6, 5), 'bracket')
    with pytest.raises(RuntimeError, match=r'^Input must be on CUDA device$'):
        base._check_mosaic(torch.zeros(6, 4))
    assert set(_mosaic.FLOAT_TAGS) == {torch.float32, torch.float16}
    assert _mosaic.out_dtype_of(None, torch.float16) is torch.float16 and _mosaic.out_dtype_of(torch.float32, torch.float16) is torch.float32
    assert _mosaic.positive_float32(0.1, 'clip') == torch.tensor(0.1).item()
    assert _mosaic.window_thresholds([1, 2.5], None) == ((1.0, 2.5), None, float('inf'))
    (t_lo, t_hi), pixel, c2 = _mosaic.window_thresholds((0.1, 0.3), 0.1)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()
    assert (t_lo, t_hi, pixel) == (f32(0.1), f32(0.3), f32(0.1)) and c2 == f32(f32(0.1) * f32(0.1))
    _mosaic.check_gains(None, torch.device('cpu'))
    for bad in ('x', torch.ones(4), torch.ones(3, dtype=torch.float64), torch.ones(6)[::2]):
        with pytest.raises(RuntimeError, match=r'^gains must be a contiguous \(3,\) float32 tensor$'):
            _mosaic.check_gains(bad, torch.device('cpu'))
    with pytest.raises(RuntimeError, match=r'^gains must be on the device of the input$'):
        _mosaic.check_gains(torch.ones(3), DEVICE)


def test_an_object_built_without_a_gpu_holds_no_buffer(td, no_gpu):
    for stage in stages(td):
        for name in ('_workspaces', '_exposures', '_work', '_states', '_buffers', '_pyramids'):
            assert len(getattr(stage, name, ())) == 0, (type(stage).__name__, name)
    p, model = td.BayerPattern.RGGB, td.NoiseModel(torch.zeros(3, 4))
    assert td.MotionHdrMerge(DEVICE, SIZE, p, model)._last is None and td.ChromaticAberration(DEVICE, SIZE, p).model is None
    assert td.TemporalDenoise(DEVICE, SIZE, p, model)._c2 == 16.0 and td.HdrMerge(DEVICE, SIZE, p, model, pixel_threshold=None)._c2 == float('inf')


def test_workspace_sizes_are_asked_once(td, no_gpu, monkeypatch):
    """Highlights, NoiseProfile and FrameStats ask the library for the size of their workspace at construction and never again."""
    p = td.BayerPattern.RGGB
    for stage in (td.Highlights(DEVICE, SIZE, p), td.NoiseProfile(DEVICE, SIZE, p), td.FrameStats(DEVICE, SIZE)):
        assert stage._workspace_bytes == stage.workspace_bytes() > 0
        asked = []
        monkeypatch.setattr(type(stage), 'workspace_bytes', lambda *a: asked.append(a) or 0)
        monkeypatch.setattr(stage._workspaces, 'get', lambda nbytes, device, key=(): nbytes)
        assert stage._workspace(DEVICE) == stage._workspace_bytes and not asked


def test_the_shared_words_stand_in_the_layer_alone():
    layer = (PACKAGE / '_mosaic.py').read_text()
    words = ('dimensions must be even (whole CFA cells)', 'radius must be 2 or 3', 'Invalid bayer pattern', 'thresholds must be (t_lo, t_hi)',
             'gains must be a contiguous (3,) float32 tensor', 'Input tensors must be all float32 or all float16', 'noise_model must be a NoiseModel, got')
    for word in words[:-1]:
        assert layer.count(word) == 1, word
    assert 'torch.cuda.current_device()' in (PACKAGE / '_stage.py').read_text() and 'torch.cuda.current_device()' not in layer
    for name in MODULES:
        text = (PACKAGE / f'{name}.py').read_text()
        for word in (*words, 'torch.cuda.current_device()', 'require_cuda_device', "def image_size"):
            assert text.count(word) == (1 if (name, word) == ('noiseprofile', words[-1]) else 0), (name, word)
        for found in re.findall(r'^_\w*TAGS = \{(.*)\}$', text, re.M):   # only a dictionary wider than FLOAT_TAGS stays with its module
            assert name in ('noiseprofile', 'framestats') and 'torch.uint16' in found, (name, found)
    text = (PACKAGE / 'pipeline' / 'image_processor.py').read_text()
    assert len(re.findall(r"is for \{stage\.image_size\}", text)) == 1 and len(re.findall(r'\b_check_mosaic_stage\(', text)) == 6
