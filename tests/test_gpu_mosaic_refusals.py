"""GPU: the refusals of the stages on raw mosaics that only a CUDA tensor reaches -- a view that is not contiguous, a float64 mosaic, a
set of frames of mixed types, gains of the wrong shape or type, fields of the wrong shape -- on a 16 x 8 mosaic, each followed by a
valid call of the same object.  What a CPU tensor reaches is the table of tests/mosaic_refusals.py."""

import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEVICE = torch.device('cuda', 0)
SIZE, HW = (16, 8), (8, 16)
CONTIGUOUS, FLOAT, FLOATS = 'Input must be contiguous', 'Input tensor must be float32 or float16', 'Input tensors must be all float32 or all float16'
OUT_DTYPE = 'out_dtype must be float32 or float16, got torch.float64'
GAINS = 'gains must be a contiguous (3,) float32 tensor'
EXPOSURES = (1.0, 0.25)


def refused(exception, message, call):
    with pytest.raises(exception) as caught:
        call()
    assert type(caught.value) is exception and re.search('^' + re.escape(message) + '$', str(caught.value.args[0])), caught.value


@pytest.fixture(scope='module')
def frames():
    torch.manual_seed(5)
    good = (torch.rand(HW, device=DEVICE) * 0.5 + 0.1).contiguous()
    return {'good': good, 'half': good.half(), 'view': torch.empty(8, 32, device=DEVICE)[:, ::2], 'double': good.double(),
            'ones': torch.ones(3, device=DEVICE)}


@pytest.fixture(scope='module')
def model(td):
    return td.NoiseModel.from_values(1e-3, 1e-5, DEVICE)


def check_output(out, dtype=torch.float32):
    assert tuple(out.shape) == HW and out.dtype == dtype and out.is_cuda and bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize('name', ['TemporalDenoise', 'MotionTemporalDenoise'])
def test_temporal(td, frames, model, name):
    stage = getattr(td, name)(DEVICE, SIZE, td.BayerPattern.RGGB, model)
    assert frames['view'].shape == HW and not frames['view'].is_contiguous()
    for exception, message, args, kwargs in (
            (RuntimeError, CONTIGUOUS, (frames['view'],), {}),
            (ValueError, OUT_DTYPE, (frames['double'],), {}),
            (RuntimeError, FLOAT, (frames['double'],), dict(out_dtype=torch.float32)),
            (RuntimeError, CONTIGUOUS, (frames['view'],), dict(gains='x')),
            (RuntimeError, GAINS, (frames['good'],), dict(gains=torch.ones(4, device=DEVICE))),
            (RuntimeError, GAINS, (frames['good'],), dict(gains=torch.ones(3, device=DEVICE, dtype=torch.float64))),
            (RuntimeError, GAINS, (frames['good'],), dict(gains=(1.0, 1.0, 1.0))),
            (RuntimeError, GAINS, (frames['good'],), dict(gains=torch.ones(6, device=DEVICE)[::2])),
            (RuntimeError, 'gains must be on the device of the input', (frames['good'],), dict(gains=torch.ones(3)))):
        refused(exception, message, lambda: stage.process(*args, **kwargs))
        check_output(stage.process(frames['good'], gains=frames['ones']))
    check_output(stage.process(frames['half'], out_dtype=torch.float16), torch.float16)
    assert int(stage.frames().item()) == 10 and list(stage._states) == [None]   # a refused call leaves the state alone


def test_motion_estimate(td, frames):
    me = td.MotionEstimate(DEVICE, SIZE)
    for exception, message, cur, ref in ((RuntimeError, CONTIGUOUS, frames['view'], frames['good']), (RuntimeError, CONTIGUOUS, frames['good'], frames['view']),
                                         (RuntimeError, FLOAT, frames['double'], frames['good']), (RuntimeError, FLOAT, frames['good'], frames['double'])):
        refused(exception, message, lambda: me.estimate(cur, ref))
        field = me.estimate(frames['good'], frames['half'])
        assert tuple(field.shape) == (1, 1, 2) and field.dtype == torch.int16 and len(me._pyramids) == 1


@pytest.mark.parametrize('name', ['HdrMerge', 'MotionHdrMerge'])
def test_brackets(td, frames, model, name):
    stage = getattr(td, name)(DEVICE, SIZE, td.BayerPattern.RGGB, model)
    good, half, view, double = frames['good'], frames['half'], frames['view'], frames['double']
    rows = [(RuntimeError, CONTIGUOUS, ([good, view],), {}),
            (RuntimeError, CONTIGUOUS, ([view, good],), {}),
            (ValueError, OUT_DTYPE, ([double, double],), {}),
            (RuntimeError, FLOATS, ([double, double],), dict(out_dtype=torch.float32)),
            (RuntimeError, FLOATS, ([good, half],), {}),
            (RuntimeError, FLOATS, ([half, good],), dict(ref=0)),
            (RuntimeError, 'exposures must be on the device of the frames', ([good, good],), dict(exposures=torch.ones(2), ref=0))]
    if name == 'MotionHdrMerge':
        fields = lambda *shape: torch.zeros(shape, dtype=torch.int16, device=DEVICE)
        wrong = 'fields must be a contiguous (2, 1, 1, 2) int16 tensor'
        rows += [(RuntimeError, wrong, ([good, good],), dict(fields=fields(1, 1, 1, 2))),
                 (RuntimeError, wrong, ([good, good],), dict(fields=fields(2, 1, 2))),
                 (RuntimeError, wrong, ([good, good],), dict(fields=fields(2, 1, 1, 4)[..., ::2])),
                 (RuntimeError, wrong, ([good, good],), dict(fields=fields(2, 1, 1, 2).int())),
                 (RuntimeError, wrong, ([good, view],), dict(fields=fields(3, 1, 1, 2))),
                 (RuntimeError, 'fields must be on the device of the frames', ([good, good],), dict(fields=fields(2, 1, 1, 2).cpu()))]
    for exception, message, args, kwargs in rows:
        kwargs = {'exposures': EXPOSURES, **kwargs}
        refused(exception, message, lambda: stage.process(*args, **kwargs))
        out, mask = stage.process([good, good * 0.25], EXPOSURES, return_mask=True)
        check_output(out)
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == HW
    check_output(stage.process(torch.stack([half, half]), EXPOSURES, out_dtype=torch.float32))
    if name == 'MotionHdrMerge':
        check_output(stage.process([good, good], EXPOSURES, fields=torch.zeros((2, 1, 1, 2), dtype=torch.int16, device=DEVICE)))
        assert stage._last == (2, DEVICE) and tuple(stage.fields().shape) == (2, 1, 1, 2)


def test_highlights_and_raw_prepare(td, frames):
    gains = frames['ones']
    for stage, float_message in ((td.Highlights(DEVICE, SIZE, td.BayerPattern.RGGB), FLOAT),
                                 (td.RawPrepare(DEVICE, SIZE, td.BayerPattern.RGGB, white=1.0), 'Input tensor must be uint16, float32 or float16')):
        for exception, message, args, kwargs in (
                (RuntimeError, CONTIGUOUS, (frames['view'], gains), {}),
                (RuntimeError, float_message, (frames['double'], gains), {}),
                (RuntimeError, CONTIGUOUS, (frames['view'], gains), dict(out_dtype=torch.float64)),
                (ValueError, OUT_DTYPE, (frames['good'], torch.ones(4, device=DEVICE)), dict(out_dtype=torch.float64)),
                (ValueError, 'white_balance must have 3 elements (R, G, B), got 4', (frames['good'], torch.ones(4, device=DEVICE)), {}),
                (ValueError, 'white_balance must have 3 elements (R, G, B), got 2', (frames['good'], (1.0, 1.0)), {})):
            refused(exception, message, lambda: stage.process(*args, **kwargs))
            check_output(stage.process(frames['good'], gains))
        check_output(stage.process(frames['half'], gains.double(), out_dtype=torch.float16), torch.float16)   # (gains of float64 are converted)
    highlights = td.Highlights(DEVICE, SIZE, td.BayerPattern.RGGB)
    refused(RuntimeError, CONTIGUOUS, lambda: highlights.chrominance(frames['view'], gains))
    refused(RuntimeError, FLOAT, lambda: highlights.statistics(frames['double'], gains))
    assert tuple(highlights.chrominance(frames['good'], gains).shape) == (3,) and len(highlights._workspaces) == 1


def test_chromatic_aberration(td, frames, model):
    ca = td.ChromaticAberration(DEVICE, SIZE, td.BayerPattern.RGGB)
    good, half, view, double = frames['good'], frames['half'], frames['view'], frames['double']
    for exception, message, args, kwargs in ((RuntimeError, CONTIGUOUS, (view,), {}), (ValueError, OUT_DTYPE, (double,), {}),
                                             (RuntimeError, FLOAT, (double,), dict(out_dtype=torch.float16)),
                                             (RuntimeError, CONTIGUOUS, (view,), dict(model=torch.zeros(2, 4)))):
        refused(exception, message, lambda: ca.correct(*args, **kwargs))
        check_output(ca.correct(good))
    for exception, message, args, kwargs in ((RuntimeError, CONTIGUOUS, ([good, view],), {}), (RuntimeError, FLOATS, (double,), {}),
                                             (RuntimeError, FLOATS, ([good, half],), {}), (RuntimeError, FLOATS, ([half, good],), dict(noise_model=model)),
                                             (RuntimeError, 'The noise model must be on the device of the input', (good,), dict(noise_model=td.NoiseModel(torch.zeros(3, 4))))):
        refused(exception, message, lambda: ca.estimate(*args, **kwargs))
        fitted = ca.estimate([good, good], noise_model=model)
        assert tuple(fitted.model.shape) == (2, 4) and fitted._workspaces is ca._workspaces
    check_output(ca.correct(half, out_dtype=torch.float32))


def test_noise_profile_and_frame_stats(td, frames, model):
    good, half, view, double = frames['good'], frames['half'], frames['view'], frames['double']
    shared = 'The frames of a set must share their dtype and device'
    profile = td.NoiseProfile(DEVICE, SIZE, td.BayerPattern.RGGB, max_frames=2)
    stats = td.FrameStats(DEVICE, SIZE, bayer_pattern=td.BayerPattern.RGGB, max_frames=2)
    for stage, call, kinds in ((profile, profile.estimate, 'float32, float16 or uint16'), (stats, stats.white_balance, 'float32, float16, uint8 or uint16')):
        for message, argument in ((CONTIGUOUS, view), (CONTIGUOUS, [good, view]), (f'Input tensor must be {kinds}', double), (shared, [good, half]),
                                  (shared, [half, good])):
            refused(RuntimeError, message, lambda: call(argument))
            call([good, good])
        assert len(stage._workspaces) == 1
    for message, kwargs in ((GAINS, dict(gains=torch.ones(4, device=DEVICE))), (GAINS, dict(gains=torch.ones(3, device=DEVICE, dtype=torch.float64))),
                            (GAINS, dict(gains=[1.0, 1.0, 1.0])), ('gains must be on the device of the input', dict(gains=torch.ones(3)))):
        refused(RuntimeError, message, lambda: model.stabilize(good, td.BayerPattern.RGGB, **kwargs))
        check_output(model.unstabilize(model.stabilize(good, td.BayerPattern.RGGB, gains=frames['ones']), td.BayerPattern.RGGB, gains=frames['ones']))
    refused(RuntimeError, CONTIGUOUS, lambda: model.stabilize(view, td.BayerPattern.RGGB))
    refused(RuntimeError, FLOAT, lambda: model.stabilize(double, td.BayerPattern.RGGB))
    refused(ValueError, OUT_DTYPE, lambda: model.unstabilize(double, td.BayerPattern.RGGB))
