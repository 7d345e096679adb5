"""CPU-only: the host layer of the frame stages (torch_darktable/_stage.py) -- the four stages bound to one frame size share its base,
the taps it makes of a sigma are the ones the restatements of Deconvolve and Defringe make, its luminance weights default to Rec. 709
as float32, an object built without a GPU holds no buffer, and no stage module calls a tdk_*_weights entry point on its own."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import deconv_spec
import defringe_spec

PACKAGE = Path(__file__).resolve().parent.parent / 'torch-darktable_amd' / 'torch_darktable'
DEVICE = torch.device('cuda', 0)
SIZE = (40, 24)


def test_the_four_sized_stages_share_the_base(td):
    from torch_darktable._stage import FrameStage
    from torch_darktable._streams import StreamBuffers

    stages = (td.ToneEqualizer(DEVICE, SIZE), td.Dehaze(DEVICE, SIZE), td.Deconvolve(DEVICE, SIZE), td.Defringe(DEVICE, SIZE),
              td.Deconvolve.from_weights(DEVICE, SIZE, (0.5, 0.25)), td.Defringe.from_weights(DEVICE, SIZE, (0.5, 0.25)))
    for stage in stages:
        assert isinstance(stage, FrameStage) and type(stage).__mro__[1] is FrameStage
        assert stage.image_size == SIZE == (stage.width, stage.height) and stage._home_device() == DEVICE
        assert type(stage)._workspace is FrameStage._workspace and type(stage).image_size is FrameStage.image_size
        assert isinstance(stage._workspaces, StreamBuffers) and stage.workspace_bytes() >= 0
    for cls in (td.Sharpen, td.Filmic, td.LMMSE):
        assert not issubclass(cls, FrameStage)
    with pytest.raises(NotImplementedError):
        FrameStage(DEVICE, SIZE).workspace_bytes()
    with pytest.raises(ValueError, match=r'^Device must be CUDA, got cpu$'):
        FrameStage(torch.device('cpu'), SIZE)
    with pytest.raises(ValueError, match=r'^Image dimensions must be 1\.\.65535, got 0x24$'):
        FrameStage(DEVICE, (0, 24))


def test_an_object_built_without_a_gpu_holds_no_buffer(td, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)   # (what the constructors ask; true of the machines without a GPU)
    for stage in (td.ToneEqualizer(DEVICE, SIZE), td.Dehaze(DEVICE, SIZE), td.Deconvolve(DEVICE, SIZE), td.Defringe(DEVICE, SIZE)):
        assert len(stage._workspaces) == 0 and stage._prepare() is None
    assert td.ToneEqualizer(DEVICE, SIZE).table is None and td.Dehaze(DEVICE, SIZE).ambient is None


@pytest.mark.parametrize('sigma', [0.5, 0.7, 1.0, 4.0 / 3.0, 2.0])
def test_taps_of_a_sigma_are_the_restatements(td, sigma):
    from torch_darktable._native import TDK_DECONV_MAX_RADIUS, TDK_DEFRINGE_MAX_RADIUS, TDK_SHARPEN_MAX_RADIUS, lib
    from torch_darktable._stage import SeparableTaps, as_float32

    sigma = as_float32(sigma)
    want = tuple(float(w) for w in deconv_spec.gaussian_taps(sigma))
    assert want == tuple(float(w) for w in defringe_spec.gaussian_taps(sigma))
    for fn, lo, hi, max_radius in ((lib.tdk_deconv_weights, 0.3, 2.0, TDK_DECONV_MAX_RADIUS), (lib.tdk_defringe_weights, 0.5, 4.0, TDK_DEFRINGE_MAX_RADIUS),
                                   (lib.tdk_sharpen_weights, 0.25, 4.0, TDK_SHARPEN_MAX_RADIUS)):
        taps = SeparableTaps.from_sigma(fn, sigma, lo, hi, max_radius)
        assert taps.values == want and taps.radius == len(want) - 1 and taps.sigma == sigma
        assert tuple(taps.c_array) == want and isinstance(taps.c_array, ctypes.Array) and repr(taps) == f'sigma={sigma:g}'
    assert td.Deconvolve(DEVICE, SIZE, sigma=sigma).taps == want == td.Defringe(DEVICE, SIZE, sigma=sigma).taps == td.Sharpen(DEVICE, sigma=sigma).weights


def test_taps_of_values_and_their_refusals(td):
    from torch_darktable._stage import SeparableTaps

    taps = SeparableTaps.from_values((0.4, 0.1 + 2 ** -30, 0.2), 6, 'taps')
    assert taps.values == tuple(float(np.float32(v)) for v in (0.4, 0.1, 0.2)) and taps.radius == 2 and taps.sigma is None
    assert repr(taps) == f'taps={taps.values}' and SeparableTaps.from_values(taps, 1, 'weights') is taps
    assert repr(SeparableTaps.from_values((0.5, 0.25), 12, 'weights')) == 'weights=(0.5, 0.25)'
    with pytest.raises(AttributeError):
        taps.other = 1
    with pytest.raises(ValueError, match=r'^weights must hold 2\.\.13 values \(radius 1\.\.12\), got 1$'):
        SeparableTaps.from_values((1.0,), 12, 'weights')
    with pytest.raises(ValueError, match=r'^taps must hold 2\.\.7 values \(radius 1\.\.6\), got 8$'):
        SeparableTaps.from_values((0.1,) * 8, 6, 'taps')
    for bad in (float('nan'), float('inf'), -0.5, 1e39):
        with pytest.raises(ValueError, match=r'^taps must be finite and >= 0, got \('):
            SeparableTaps.from_values((0.5, bad), 6, 'taps')
    from torch_darktable._native import lib
    for sigma in (0.29, 2.01, float('nan')):
        with pytest.raises(ValueError, match=r'^sigma must lie in \[0\.3, 2\], got '):
            SeparableTaps.from_sigma(lib.tdk_deconv_weights, sigma, 0.3, 2.0, 6)
    with pytest.raises(ValueError, match=r'^tdk_deconv_weights: sigma must lie in \[0\.3, 2\]$'):   # the library's own refusal comes through
        SeparableTaps.from_sigma(lib.tdk_deconv_weights, 2.5, 0.3, 4.0, 6)


def test_luma_weights_default_to_rec709_as_float32(td):
    from torch_darktable import _stage

    rec709 = tuple(float(np.float32(v)) for v in (0.2126, 0.7152, 0.0722))
    values, array = _stage.luma_weights(None)
    assert values == rec709 == tuple(array) and _stage.REC709 == deconv_spec.REC709
    assert _stage.luma_weights([1, 0.1, 0])[0] == (1.0, float(np.float32(0.1)), 0.0)
    assert td.ToneEqualizer(DEVICE, SIZE).weights == td.Dehaze(DEVICE, SIZE).weights == td.Deconvolve(DEVICE, SIZE).weights == td.Filmic(DEVICE).weights == rec709
    for bad in ((1, 2), (1, 2, 3, 4), (1, float('nan'), 0), (1, -1e-9, 0), (float('inf'), 0, 0)):
        with pytest.raises(ValueError, match=r'^weights must be three finite values >= 0, got \('):
            _stage.luma_weights(bad)
    assert _stage.as_float32(0.1) == float(np.float32(0.1)) and _stage.as_float32(1e39) == float('inf') and _stage.as_float32(3) == 3.0


def test_only_the_layer_fills_tap_buffers_and_names_rec709():
    """The buffer `ctypes.c_float * (max_radius + 1)` and the call of a tdk_*_weights entry point that fills it stand in the layer alone:
    a stage hands its entry point to SeparableTaps.from_sigma and spells no ctypes itself."""
    layer = (PACKAGE / '_stage.py').read_text()
    assert re.search(r'ctypes\.c_float \* \(max_radius \+ 1\)\)\(\).*?\n\s+if weights_fn\(sigma, buf, ', layer, re.S)
    users = {}
    for name in ('sharpen', 'deconvolve', 'defringe', 'toneequal', 'dehaze', 'filmic', 'lmmse'):
        text = (PACKAGE / f'{name}.py').read_text()
        assert 'ctypes' not in text and 'torch.cuda.current_device()' not in text, name
        users[name] = re.findall(r'([\w.]+)\(lib\.(tdk_\w+_weights)\b', text)
        assert len(re.findall(r'tdk_\w+_weights\b', text)) == len(users[name]), name
    assert users == {'sharpen': [('SeparableTaps.from_sigma', 'tdk_sharpen_weights')], 'deconvolve': [('SeparableTaps.from_sigma', 'tdk_deconv_weights')],
                     'defringe': [('SeparableTaps.from_sigma', 'tdk_defringe_weights')], 'toneequal': [], 'dehaze': [], 'filmic': [], 'lmmse': []}
    for path in sorted(PACKAGE.glob('*.py')):
        assert bool(re.search(r'^REC709 = ', path.read_text(), re.M)) == (path.name == '_stage.py'), path.name
