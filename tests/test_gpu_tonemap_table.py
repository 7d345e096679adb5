"""GPU: the table form of the Reinhard tone mapper for binary16 frames (include/tdk_hip_tables.h, csrc/tonemap.hip: tonemap_table +
tonemap_apply_table) against the per-pixel kernels it stands in for.

reinhard_tonemap of a float16 frame with vibrance 0 and 0 < 1 / gamma <= 2 fills a table of the output byte of every (channel,
binary16 code) and the pixels take their bytes from it; verification_paths(tonemap_direct=True) runs the per-pixel kernels on the
same call ('tdk_tonemap(direct)' in the library's event timer), which are the kernels every other case runs.  While map_key is
below 1 the per-pixel kernel is one function of a sample and the constants, so the bytes must be equal for every code, NaN and the
infinities included.  With map_key on its clamp (metrics[0] <= -9.21034) and negative samples it picks its arithmetic form per thread
(all of a thread's groups once one of them holds a negative sample), the table per code: there a byte at a rounding tie may differ
by 1; without a negative sample the two are equal again.

The frame of the 'every code' tests is 256 x 256: each channel holds each of the 65 536 codes once, in its own order, so a pixel
joins three unrelated codes and a thread's four pixels twelve."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TABLE, APPLY, DIRECT = 'tdk_tonemap(table)', 'tdk_tonemap', 'tdk_tonemap(direct)'
ORDINARY = (-2.0, 0.2, 0.25, 0.2, 0.15)          # log mean, mean grey, mean r, g, b
NAN_MEAN = (-2.0, 0.2, 0.25, float('nan'), 0.15)
NEGATIVE_MEAN = (-2.0, 0.2, -0.1, 0.2, 0.15)
ON_CLAMP = -9.3                                  # a log mean at or below -9.21034: map_key == 1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def codes_frame(dev, codes):
    """(len(codes) / 256, 256, 3) float16: every channel holds every code of `codes` once, each channel in its own order."""
    rng = np.random.default_rng(20240)
    planes = [rng.permutation(codes.astype(np.uint16)) for _ in range(3)]
    bits = np.stack(planes, axis=-1).reshape(-1, 256, 3)
    x = torch.empty(bits.shape, dtype=torch.float16, device=dev)
    x.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)))   # the bits as they are: no conversion touches a NaN's payload
    return x


@pytest.fixture(scope='module')
def every_code(dev):
    x = codes_frame(dev, np.arange(65536))
    seen = x.view(torch.int16).to(torch.int32).cpu().numpy() & 0xffff
    assert all(np.array_equal(np.sort(seen[..., c].ravel()), np.arange(65536)) for c in range(3))
    assert not np.array_equal(seen[..., 0], seen[..., 1]) and not np.array_equal(seen[..., 1], seen[..., 2])
    return x


def params(td, gamma=None, light_adapt=None, vibrance=None):
    from torch_darktable.pipeline import ImageProcessingSettings

    s = ImageProcessingSettings()
    return td.TonemapParameters(s.tone_gamma if gamma is None else gamma, s.tone_intensity, s.light_adapt if light_adapt is None else light_adapt,
                                s.vibrance if vibrance is None else vibrance)


def metrics_of(dev, values):
    return torch.tensor(values, dtype=torch.float32, device=dev)


def timed(fn):
    """(result, {timer name: launches}) of one call under the library's event timer."""
    from torch_darktable import _native

    _native.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = {k: v[0] for k, v in _native.profile_report().items()}
    finally:
        _native.profile_enable(False)
    return out, names


def direct(td, fn):
    from torch_darktable.torch_darktable_extension import verification_paths

    with verification_paths(tonemap_direct=True):
        return fn()


SETTINGS = [{}] + [{'gamma': g} for g in (0.5, 1.0, 2.2)] + [{'light_adapt': a} for a in (0.0, 0.5, 1.0)]


@pytest.mark.parametrize('metrics', [ORDINARY, NAN_MEAN, NEGATIVE_MEAN], ids=['ordinary', 'nan mean', 'negative mean'])
@pytest.mark.parametrize('setting', SETTINGS, ids=lambda s: ','.join(f'{k}={v}' for k, v in s.items()) or 'defaults')
def test_every_code_gives_the_bytes_of_the_per_pixel_kernel(td, dev, every_code, setting, metrics):
    p, m = params(td, **setting), metrics_of(dev, metrics)
    got, names = timed(lambda: td.reinhard_tonemap(every_code, m, p))
    want, direct_names = timed(lambda: direct(td, lambda: td.reinhard_tonemap(every_code, m, p)))
    assert names == {TABLE: 1, APPLY: 1}, names               # the table form ran ...
    assert direct_names == {DIRECT: 1}, direct_names          # ... and the other call did not take it
    assert got.dtype == torch.uint8 and got.shape == every_code.shape
    differing = (got != want).sum().item()
    print(setting, metrics, 'differing bytes:', differing, 'distinct bytes:', want.unique().numel())
    assert torch.equal(got, want), (setting, metrics, differing)
    assert want.unique().numel() > 2   # the comparison is of a tone curve, not of a constant frame


@pytest.mark.parametrize('metrics', [ORDINARY, NEGATIVE_MEAN], ids=['ordinary', 'negative mean'])
def test_key_on_its_clamp_without_a_negative_sample_is_equal(td, dev, metrics):
    """No negative sample: with an ordinary mean neither form takes the exact arithmetic, with a mean that may be negative both
    take it for every sample -- equal bytes either way."""
    x = codes_frame(dev, np.arange(32768))   # sign bit clear: +0 .. 65504, +inf, the positive NaNs
    p, m = params(td), metrics_of(dev, (ON_CLAMP,) + metrics[1:])
    got, names = timed(lambda: td.reinhard_tonemap(x, m, p))
    want = direct(td, lambda: td.reinhard_tonemap(x, m, p))
    assert names == {TABLE: 1, APPLY: 1}, names
    assert torch.equal(got, want), (got != want).sum().item()


def test_key_on_its_clamp_with_negative_samples_differs_by_one_step_at_most(td, dev, every_code):
    p, m = params(td), metrics_of(dev, (ON_CLAMP,) + ORDINARY[1:])
    got = td.reinhard_tonemap(every_code, m, p)
    want = direct(td, lambda: td.reinhard_tonemap(every_code, m, p))
    d = (got.to(torch.int16) - want.to(torch.int16)).abs()
    share = (d != 0).float().mean().item()
    print(f'key on its clamp, every code: {share:.3e} of the bytes differ, largest difference {d.max().item()}')
    assert d.max().item() <= 1, f'largest difference {d.max().item()}, {share:.3e} of the bytes differ'


@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (7, 9)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_small_frames_and_pixel_tails(td, dev, every_code, shape):
    """H W % 4 != 0: the pixels past the last group of four go through the per-pixel tail kernel; 1 x 1 has no group at all."""
    h, w = shape
    x = every_code.reshape(-1, 3)[1000:1000 + h * w].reshape(h, w, 3).clone()
    p, m = params(td), metrics_of(dev, ORDINARY)
    got, names = timed(lambda: td.reinhard_tonemap(x, m, p))
    want = direct(td, lambda: td.reinhard_tonemap(x, m, p))
    assert names == ({TABLE: 1, APPLY: 2} if h * w >= 4 else {APPLY: 1}), names
    assert got.shape == (h, w, 3) and torch.equal(got, want)


def test_a_view_that_is_not_contiguous(td, dev, every_code):
    x = every_code[10:74, 100:228:2]   # 64 x 64, a stride of two pixels
    assert x.shape == (64, 64, 3) and not x.is_contiguous()
    p, m = params(td), metrics_of(dev, ORDINARY)
    got, names = timed(lambda: td.reinhard_tonemap(x, m, p))
    assert names == {TABLE: 1, APPLY: 1}, names
    assert torch.equal(got, direct(td, lambda: td.reinhard_tonemap(x, m, p)))
    assert torch.equal(got, td.reinhard_tonemap(x.contiguous(), m, p))


NOT_TAKEN = {
    'float32 input': lambda td, x, m: td.reinhard_tonemap(x.float(), m, params(td)),
    'aces': lambda td, x, m: td.aces_tonemap(x, params(td)),
    'adaptive aces': lambda td, x, m: td.aces_tonemap(x, params(td), m),
    'linear': lambda td, x, m: td.linear_tonemap(x, m, params(td)),
    'vibrance 0.3': lambda td, x, m: td.reinhard_tonemap(x, m, params(td, vibrance=0.3)),
    'gamma 0.4': lambda td, x, m: td.reinhard_tonemap(x, m, params(td, gamma=0.4)),
}


@pytest.mark.parametrize('case', list(NOT_TAKEN))
def test_the_other_cases_run_the_per_pixel_kernels(td, dev, every_code, case):
    """float32 storage, the other three mappers, vibrance != 0 and 1 / gamma > 2 have no table form: the per-pixel kernels run under
    their own timer name, and the bytes are those of the same call with the table form switched off."""
    m = metrics_of(dev, ORDINARY)
    got, names = timed(lambda: NOT_TAKEN[case](td, every_code, m))
    assert names == {APPLY: 1}, (case, names)
    assert torch.equal(got, direct(td, lambda: NOT_TAKEN[case](td, every_code, m))), case


def test_two_streams_keep_their_own_tables(td, dev, every_code):
    """One frame per stream with its own metrics, the calls interleaved: a table shared between the streams would hand one frame
    the other's bytes."""
    p = params(td)
    frames = [every_code[:64, :64].contiguous(), every_code[64:128, 64:128].contiguous()]
    metrics = [metrics_of(dev, ORDINARY), metrics_of(dev, (-6.0, 0.02, 0.01, 0.03, 0.02))]
    want = [direct(td, lambda: td.reinhard_tonemap(f, m, p)) for f, m in zip(frames, metrics)]
    assert not torch.equal(td.reinhard_tonemap(frames[0], metrics[1], p), want[0])   # the metrics matter
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    outs = []
    for _ in range(50):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                outs.append((k, td.reinhard_tonemap(frames[k], metrics[k], p)))
    torch.cuda.synchronize()
    wrong = [i for i, (k, o) in enumerate(outs) if not torch.equal(o, want[k])]
    assert not wrong, wrong


def test_captured_in_a_graph(td, dev, every_code):
    from torch_darktable.sharding import FrameStreams

    p = params(td)
    m = metrics_of(dev, ORDINARY)
    frames = [every_code[:64, :64].contiguous(), every_code[64:128, 64:128].contiguous()]
    eager = [td.reinhard_tonemap(f, m, p) for f in frames]
    runner = FrameStreams(dev, lambda: (lambda f: td.reinhard_tonemap(f, m, p)), streams=2)
    batch = runner.capture(frames)
    for o in batch.outputs:
        o.zero_()
    outs = batch.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert torch.equal(o, e)
    fresh = [every_code[128:192, :64].contiguous(), every_code[192:256, 64:128].contiguous()]   # the replay reads the static inputs as they are now
    outs = batch.replay(fresh)
    torch.cuda.synchronize()
    for o, f in zip(outs, fresh):
        assert torch.equal(o, td.reinhard_tonemap(f, m, p))
