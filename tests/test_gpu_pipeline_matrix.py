"""ImageProcessor, as a user builds it from a preset, a camera file or hand-set flags, against the oracle chain of
tests/pipeline_chain.py: every branch of load_image, process_rgb, tonemap and transform that the settings select.

The comparison runs stage by stage (demosaiced frame, bounds, pre-tonemap float image, metrics, the tone mapper on the GPU's own
input, then end to end and against the by-hand composition of the public stages), because the reference's adaptive mappers are
discontinuous at a zero channel when light_adapt == 1: there an end-to-end uint8 comparison is ill conditioned, while the float
image in front of the mapper and the mapper on identical input are not.  tests/test_pipeline_chain.py holds, on the oracle alone,
that the end-to-end bound used here leaves a factor of 2 over what the reference's own sensitivity to 2 TOL shows, and measures
the float16 bound.

Measured on an MI355X: end to end at most 1 LSB on at most 2.0e-4 of the values of a frame in float32 (bound: 1 LSB, 0.02); with
float16 storage every configuration of group D gives exactly the (maximum, share above 1 LSB) that rounding the stored images to
binary16 does to the oracle chain (tests/test_pipeline_chain.py), so the bound of maximum + 1 LSB and twice the share holds with
that margin.  The slowest case takes 0.6 s (the first one: it loads the library), every other under 0.15 s."""

import numpy as np
import pytest
import torch

import pipeline_chain as pc
from pipeline_chain import F16_CONFIGS, F32_CONFIGS, TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def gpu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def make_processor(td, cfg, dev, settings=None):
    from torch_darktable.pipeline import ImageProcessor, ImageTransform

    if cfg.camera is not None and settings is None:   # group B: the way a camera file becomes a processor
        cs = cfg.camera
        assert (cs.bayer_pattern.name, cs.packed_format.name, cs.padding, cs.white_balance) == (cfg.pattern, cfg.packed_format, cfg.padding, cfg.white_balance)
        return ImageProcessor.from_camera_settings(cs, dev, storage_dtype=cfg.storage_dtype)
    tf = {n: ImageTransform[t] for n, t in cfg.transform.items()} if isinstance(cfg.transform, dict) else ImageTransform[cfg.transform]
    return ImageProcessor(cfg.size, td.BayerPattern[cfg.pattern], td.PackedFormat[cfg.packed_format], settings if settings is not None else cfg.settings,
                          dev, cfg.white_balance, tf, padding=cfg.padding, storage_dtype=cfg.storage_dtype)


def expected_shape(cfg, name):
    from torch_darktable.pipeline import ImageTransform, transformed_size

    w, h = transformed_size(cfg.size, ImageTransform[cfg.transform_of(name)])
    return (h, w, 3)


def u8_diff(a, b):
    return np.abs(a.astype(np.int32) - b.astype(np.int32))


@pytest.mark.parametrize('cfg', F32_CONFIGS, ids=lambda c: c.name)
def test_processor_against_oracle_chain(td, oracle, dev, scene, cfg):
    from torch_darktable.tonemap import MetricsAccumulator

    post, bound = cfg.settings.postprocess, cfg.green_bound
    proc, stages = make_processor(td, cfg, dev), make_processor(td, cfg, dev)
    for call, (packed, ref) in enumerate(pc.reference(oracle, scene, cfg)):
        where = f'{cfg.name} call {call}'
        raw = {n: gpu(p, dev) for n, p in packed.items()}
        assert all(b.numel() == proc.expected_bytes for b in raw.values())
        out = proc.process_image_set(raw)
        assert list(out.keys()) == list(cfg.names)

        # 2. bounds, 4. metrics (after the moving average)
        if post:
            assert np.allclose(npy(proc.bounds), ref['bounds'], rtol=bound, atol=0), (where, npy(proc.bounds), ref['bounds'])
        else:
            assert np.array_equal(npy(proc.bounds), ref['bounds']), (where, npy(proc.bounds), ref['bounds'])
        assert np.allclose(npy(proc.metrics), ref['metrics'], rtol=2e-5, atol=1e-7), (where, npy(proc.metrics), ref['metrics'])

        acc = MetricsAccumulator(dev, stride=8)
        for n in cfg.names:
            # 1. the demosaiced frame
            img = stages.load_image(raw[n])
            got, want = npy(img), ref['demosaiced'][n]
            assert img.dtype == torch.float32 and got.shape == want.shape
            if post:   # R and B never see the green ratio; G differs by the association order of two fp32 sums
                assert np.array_equal(got[:, :, 0::2], want[:, :, 0::2]), where
                assert np.allclose(got[:, :, 1], want[:, :, 1], rtol=bound, atol=0), (where, np.abs(got[:, :, 1] - want[:, :, 1]).max())
            else:
                assert np.array_equal(got, want), (where, n, int((got != want).sum()))

            # 3. the float image in front of the tone mapper, by the public stages
            pre = stages.process_rgb(img, proc.bounds, acc)
            got, want = npy(pre), ref['pre'][n]
            err = np.abs(got - want)
            if post:
                assert (err <= 2 * TOL + bound * np.abs(want)).all(), (where, n, float(err.max()))
            elif cfg.stages == 'neither':   # the same fp32 expression (test_normalize_image_kernel)
                assert np.array_equal(got, want), (where, n, float(err.max()))
            else:
                assert err.max() <= 2 * TOL, (where, n, float(err.max()))

            # 5. the tone mapper on its own input: every pixel, the zero channels with their 0 / 0 included
            u8 = stages.tonemap(pre, proc.metrics)
            d = u8_diff(npy(u8), pc.tonemap(oracle, cfg, got, npy(proc.metrics)))
            assert u8.dtype == torch.uint8 and d.max() <= 1 and (d > 0).mean() < 2e-3, (where, n, int(d.max()), float((d > 0).mean()), int((d > 1).sum()))

            # 7. the result is the composition of the public stages
            assert tuple(out[n].shape) == expected_shape(cfg, n) and out[n].dtype == torch.uint8 and out[n].is_contiguous()
            assert torch.equal(out[n], stages.transform(u8, n)), (where, n)

            # 6. end to end, outside the pixels where the reference is discontinuous
            mask = pc.orient(pc.ill_conditioned(cfg, ref['pre'][n]), cfg.transform_of(n))
            assert mask.mean() <= 0.05 and (cfg.group not in 'AB' or not mask.any()), (where, n, float(mask.mean()))
            d = u8_diff(npy(out[n]), ref['out'][n])[~mask]
            print(f'{where} {n}: end to end max {d.max()} share {(d > 0).mean():.5f} masked {mask.mean():.4f}')
            assert d.max() <= 1 and (d > 0).mean() < 0.02, (where, n, int(d.max()), float((d > 0).mean()))
        # the accumulator of the by-hand stages saw what the processor's saw (first call: no history in the average)
        if call == 0:
            assert torch.allclose(acc.finish(), proc.metrics, rtol=1e-6, atol=0), where


@pytest.mark.parametrize('cfg', F16_CONFIGS, ids=lambda c: c.name)
def test_float16_storage_against_oracle_chain(td, oracle, dev, scene, cfg):
    """float16 storage between the stages: against the float32 oracle chain within what rounding the stored images to binary16 does
    to the oracle chain itself (pipeline_chain.f16_bound: that maximum + 1 LSB, twice that share above 1 LSB), and equal to the
    composition of the public stages."""
    worst, share = pc.f16_bound(oracle, scene, cfg)
    proc, stages = make_processor(td, cfg, dev), make_processor(td, cfg, dev)
    for call, (packed, ref) in enumerate(pc.reference(oracle, scene, cfg)):
        raw = {n: gpu(p, dev) for n, p in packed.items()}
        out = proc.process_image_set(raw)
        for n in cfg.names:
            img = stages.load_image(raw[n])
            pre = stages.process_rgb(img, proc.bounds)
            assert img.dtype == torch.float16 and pre.dtype == torch.float16
            assert out[n].dtype == torch.uint8 and tuple(out[n].shape) == expected_shape(cfg, n)
            assert torch.equal(out[n], stages.transform(stages.tonemap(pre, proc.metrics), n)), (cfg.name, n)
            mask = pc.orient(pc.ill_conditioned(cfg, ref['pre'][n]), cfg.transform_of(n))
            assert mask.mean() <= 0.05 and (cfg.name[:2] != 'D-' or not mask.any())
            d = u8_diff(npy(out[n]), ref['out'][n])[~mask]
            print(f'{cfg.name} {n}: max {d.max()} (bound {worst}) share(> 1 LSB) {(d > 1).mean():.2e} (bound {share:.2e}) hist {np.bincount(d.ravel())}')
            assert d.max() <= worst and (d > 1).mean() <= share, (cfg.name, n, int(d.max()), float((d > 1).mean()), worst, share)


# ---------------------------------------------------------------------------------------------------------------- update_settings
def _s(**kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ToneMapper

    base = dict(moving_average=1.0, light_adapt=0.8, vibrance=0.3, tone_gamma=2.2, tone_intensity=1.0, enable_denoise=True, enable_bilateral=True,
                tone_mapping='aces', debayer='rcd')
    base.update(kw)
    base['debayer'], base['tone_mapping'] = Debayer[base['debayer']], ToneMapper[base['tone_mapping']]
    return ImageProcessingSettings(**base)


UPDATES = {
    'bilateral sigmas': (dict(), dict(bil_sigma_spatial=3.0, bil_sigma_luminance=0.1)),
    'bilateral sigmas, stage alone': (dict(enable_denoise=False), dict(enable_denoise=False, bil_sigma_spatial=1.0, bil_sigma_luminance=0.3)),
    'ppg_median_threshold': (dict(debayer='ppg'), dict(debayer='ppg', ppg_median_threshold=0.02)),
    'post-process parameters': (dict(postprocess=True), dict(postprocess=True, color_smoothing_passes=1, green_eq_threshold=0.1)),
    'denoise -> bilateral': (dict(enable_bilateral=False), dict(enable_denoise=False)),
    'both -> neither': (dict(), dict(enable_denoise=False, enable_bilateral=False)),
    'neither -> both': (dict(enable_denoise=False, enable_bilateral=False), dict()),
    'tone_mapping': (dict(), dict(tone_mapping='adaptive_aces')),
    'debayer rcd -> ppg': (dict(), dict(debayer='ppg')),
    'debayer bilinear -> rcd': (dict(debayer='bilinear'), dict()),
    'postprocess on': (dict(), dict(postprocess=True)),
    'postprocess off': (dict(postprocess=True, debayer='ppg'), dict(debayer='ppg')),
}


@pytest.mark.parametrize('group', list(UPDATES), ids=lambda g: g.replace(' ', '_'))
def test_update_settings_equals_a_fresh_processor(td, oracle, dev, scene, group):
    """Settings X, one frame, update_settings(Y), the frame again: what a processor built with Y gives, and not what X gave (a
    workspace that update_settings left stale would give X's picture, or a mixture)."""
    x, y = (_s(**kw) for kw in UPDATES[group])
    cfg = pc.Config(name='update', group='U', settings=x, white_balance=(1.5, 1.0, 1.2), padding=64, transform='rotate_90', seed=333)
    raw = gpu(pc.frames(oracle, scene, cfg, 0)['cam'], dev)
    proc = make_processor(td, cfg, dev)
    first = proc.process(raw, 'cam').clone()
    proc.update_settings(y)
    assert proc.settings == y
    # the moving averages are state of the frames seen, not of the settings: a + (b - a) * 1 is b only up to an fp32 rounding
    proc.bounds = proc.metrics = None
    second = proc.process(raw, 'cam')
    fresh = make_processor(td, cfg, dev, settings=y).process(raw, 'cam')
    assert torch.equal(second, fresh), (group, int((second != fresh).sum()))
    assert not torch.equal(second, first), group
    assert torch.equal(first, make_processor(td, cfg, dev).process(raw, 'cam')), group   # and X's result was X's
    # and back again
    proc.update_settings(x)
    proc.bounds = proc.metrics = None
    assert torch.equal(proc.process(raw, 'cam'), first), group


# ---------------------------------------------------------------------------------------------------------------- error path
@pytest.mark.parametrize('debayer', ['rcd', 'ppg', 'bilinear'])
@pytest.mark.parametrize('padding', [0, 64])
def test_wrong_byte_count_is_refused(td, oracle, dev, scene, debayer, padding):
    """The branches of load_image a configuration without optional stages reaches (the fused RCD head; decode + demosaic), with
    and without trailing padding: a buffer of another length never reaches a kernel."""
    from torch_darktable.pipeline.image_processor import ImageSizeMismatchError

    cfg = pc.Config(name='error', group='E', settings=_s(debayer=debayer), white_balance=(1.5, 1.0, 1.2), padding=padding, seed=334)
    raw = gpu(pc.frames(oracle, scene, cfg, 0)['cam'], dev)
    proc = make_processor(td, cfg, dev)
    w, h = cfg.size
    assert proc.expected_bytes == raw.numel() == w * h * 3 // 2 + padding
    wrong = [raw[:-1], torch.cat([raw, raw[:1]]), raw[:0]]
    if padding:
        wrong.append(raw[:-padding])   # the bare payload of a padded camera
    for bad in wrong:
        for call in (lambda: proc.load_image(bad), lambda: proc.process(bad, 'cam'), lambda: proc.process_image_set({'a': raw, 'b': bad})):
            with pytest.raises(ImageSizeMismatchError) as ei:
                call()
            assert ei.value.image_size == cfg.size and ei.value.padding == padding and ei.value.packed_format == td.PackedFormat.Packed12
            assert f'got {bad.numel()} bytes' in str(ei.value) and f'expected {raw.numel()} bytes' in str(ei.value)
    assert proc.process(raw, 'cam').shape == (h, w, 3)   # the refused calls left the processor usable
