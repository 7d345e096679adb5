"""What tests/test_gpu_pipeline_matrix.py relies on, measured on the CPU oracle alone.

The GPU tests compare ImageProcessor with the oracle chain of tests/pipeline_chain.py end to end on uint8.  That comparison only
means something where the reference itself is well conditioned: where an input difference the float stages are allowed (2 TOL)
cannot move the uint8 result by more than a rounding.  These tests perturb the oracle's own pre-tonemap image by +-2 TOL and hold
the outcome to half of what the GPU tests allow, outside the pixels `ill_conditioned` marks.

Measured worst values over the float32 CONFIGS (every frame of every call, three draws each):
  (a) largest move outside the mask            1 LSB      (asserted <= 1)
  (b) share of moved values outside the mask   0.0071     (asserted <= 0.01; the GPU tests allow 0.02)
  (c) mask share of a frame, at 2 TOL          0.0255     (asserted <= 0.05; empty for groups A and B)
The second call of group B is darker by 0.75: at 0.55, the EMA test's factor, (b) reaches 0.0126 on the camera files' gamma 2.0, and
plain ACES moves by 3 LSB at its zero crossing (rrt_odt is negative below 0.0032).  Row C05 runs on a scene of its own
(pipeline_chain._C_SEEDS).

float16 storage (group D): the oracle chain in float32 against the chain rounded to binary16 where the pipeline stores images,
(largest uint8 difference, share of values above 1 LSB):
  D-aces                                (3, 8.1e-05)   128 x 96, the configuration test_image_processor_end_to_end bounds by (4, 5e-4)
  D-adaptive_aces                       (4, 1.0e-04)
  D-reinhard                            (1, 0)
  D01-ppg+pp-both-reinhard-BGGR         (2, 6.8e-05)
  D03-rcd+pp-both-adaptive_aces-GBRG    (2, 1.4e-04)
  D09-bilinear-bilateral-reinhard-BGGR  (2, 6.8e-05)
The GPU bound is that maximum plus 1 LSB and twice that share (pipeline_chain.f16_bound).  The figure depends on the scene: for the
aces preset it runs from 1 to 11 LSB over scenes 310 .. 325 (a rounded value flips a colour-smoothing median), so D-aces has a
scene on which the reference's own figure plus 1 LSB stays inside the bound the suite already holds that configuration to."""

import numpy as np
import pytest

import pipeline_chain as pc
from pipeline_chain import CONFIGS, F16_CONFIGS, F32_CONFIGS, TABLE_C, TOL


def test_table_covers_its_pairs():
    """Every value of every axis of table C, and every pair the table is written for, so that it cannot shrink quietly."""
    rows = TABLE_C
    deb, post, stages, mapper, pattern, gains, fmt, pad, tf, la = (list(col) for col in zip(*rows))
    debayers, mappers, patterns = ['bilinear', 'ppg', 'rcd'], ['linear', 'reinhard', 'aces', 'adaptive_aces'], ['RGGB', 'BGGR', 'GRBG', 'GBRG']
    assert set(deb) == set(debayers) and set(post) == {False, True} and set(stages) == set(pc.STAGES) and set(mapper) == set(mappers)
    assert set(pattern) == set(patterns) and None in gains and any(g is not None for g in gains)
    assert set(fmt) == {'Packed12', 'Packed12_IDS'} and set(pad) == {0, 64} and set(tf) == set(pc.TRANSFORMS)

    def pairs(a, b):
        return set(zip(a, b))

    assert pairs(deb, stages) == {(d, s) for d in debayers for s in pc.STAGES}
    assert pairs(deb, pattern) == {(d, p) for d in debayers for p in patterns}
    assert pairs(deb, post) == {(d, p) for d in debayers for p in (False, True)}
    assert pairs(stages, mapper) == {(s, m) for s in pc.STAGES for m in mappers}
    # white_balance=None through the fused RCD head, and a padded payload through it
    assert ('rcd', None) in pairs(deb, gains) and ('rcd', 64) in pairs(deb, pad) and ('ppg', 64) in pairs(deb, pad)
    c = [x for x in CONFIGS if x.group == 'C']
    assert len(c) == len(rows) and sum(x.settings.debayer.name == 'ppg' and x.settings.ppg_median_threshold > 0 for x in c) == 1
    default = [x for x in c if x.settings.light_adapt == 1.0]
    assert len(default) >= 3 and all(x.settings.light_adapt == 0.8 for x in c if x not in default)
    assert any(x.settings.tone_mapping.name == 'adaptive_aces' and x.stages == 'both' for x in default)
    assert {x.size for x in CONFIGS} == {pc.SMALL, pc.SMALL_B} and sum(x.size == pc.SMALL_B for x in F32_CONFIGS) == 3
    # A as shipped but for the moving average; B as in the files but for the size; D = A and three rows of C
    from torch_darktable.pipeline import presets
    for name, s in presets.items():
        a = next(x for x in CONFIGS if x.name == f'A-{name}')
        assert a.settings == s.model_copy(update={'moving_average': 1.0}) and s.vibrance == 0.5
    b = [x for x in CONFIGS if x.group == 'B']
    assert len(b) == 4 and all(x.calls == 2 and len(x.names) == 2 and x.settings.moving_average == 0.02 for x in b)
    assert sum(isinstance(x.transform, dict) for x in b) == 1 and sum(x.ids for x in b) == 2 and sum(x.padding > 0 for x in b) == 1
    assert len(F16_CONFIGS) == 6


def test_reference_conditions(oracle, scene):
    """(a) - (c) of the module docstring, on the reference alone."""
    worst_move, worst_share, worst_mask = 0, 0.0, 0.0
    for cfg in F32_CONFIGS:   # group D runs the chains of A and of three rows of C
        lab = cfg.stages != 'neither'
        for call, (_, ref) in enumerate(pc.reference(oracle, scene, cfg)):
            for k, name in enumerate(cfg.names):
                pre, base = ref['pre'][name], ref['u8'][name].astype(np.int32)
                mask = pc.ill_conditioned(cfg, pre)
                keep = ~np.broadcast_to(mask[:, :, None], pre.shape)
                if cfg.group in 'AB':
                    assert not mask.any(), cfg.name
                assert mask.mean() <= 0.05, (cfg.name, call, name, mask.mean())
                worst_mask = max(worst_mask, float(mask.mean()))
                for draw in range(3):
                    rng = np.random.default_rng(1000 * draw + 10 * call + k)
                    x = pre + rng.uniform(-2 * TOL, 2 * TOL, pre.shape).astype(np.float32)
                    if lab:   # modify_luminance clips its result to [0, 1]
                        x = np.clip(x, 0.0, 1.0)
                    d = np.abs(pc.tonemap(oracle, cfg, x.astype(np.float32), ref['metrics']).astype(np.int32) - base)[keep]
                    assert d.max() <= 1, (cfg.name, call, name, draw, int(d.max()), int((d > 1).sum()))
                    assert (d > 0).mean() <= 0.01, (cfg.name, call, name, draw, float((d > 0).mean()))
                    worst_move, worst_share = max(worst_move, int(d.max())), max(worst_share, float((d > 0).mean()))
    print(f'\nreference conditions: (a) max move {worst_move} LSB  (b) share moved {worst_share:.5f}  (c) mask share {worst_mask:.5f}')


def test_adaptive_aces_zero_channel_trap(oracle):
    """The discontinuity the mask is there for: at light_adapt = 1 a channel that is exactly 0 blackens the whole pixel."""
    px = np.array([[[0.5, 0.0, 0.3], [0.5, 1e-5, 0.3]]], np.float32)
    m = np.array([np.log(0.4), 0.4, 0.45, 0.4, 0.35], np.float32)   # a mid-grey scene; at light_adapt = 1 only the log mean acts
    at1 = oracle.tonemap('adaptive_aces', px, m, 2.2, 1.0, 1.0, 0.3)
    assert at1[0, 0].tolist() == [0, 0, 0] and at1[0, 1].tolist() == [213, 0, 180]
    at08 = oracle.tonemap('adaptive_aces', px, m, 2.2, 1.0, 0.8, 0.3).astype(np.int32)
    assert np.abs(at08[0, 0] - at08[0, 1]).max() <= 1 and at08[0, 0].max() > 100
    cfg = next(c for c in CONFIGS if c.settings.tone_mapping.name == 'adaptive_aces' and c.settings.light_adapt == 1.0)
    assert pc.ill_conditioned(cfg, px).tolist() == [[True, True]]
    assert not pc.ill_conditioned(next(c for c in CONFIGS if c.name == 'A-adaptive_aces'), px).any()


@pytest.mark.parametrize('cfg', F16_CONFIGS, ids=lambda c: c.name)
def test_float16_bound_from_the_reference(oracle, scene, cfg):
    worst, share = pc.f16_measure(oracle, scene, cfg)
    bound = pc.f16_bound(oracle, scene, cfg)
    print(f'\n{cfg.name}: float32 chain vs binary16-rounded chain: max {worst} LSB, share(> 1 LSB) {share:.2e}; GPU bound {bound}')
    # rounding a [0, 1] image to binary16 moves it by at most 2^-12: a few LSB after the tone curve, never a different picture
    assert 1 <= worst <= 8 and share <= 5e-3
    assert bound[0] <= worst + 1 and bound[1] <= 2 * share
    if cfg.name in pc.F16_ALREADY_BOUNDED:   # the existing bound holds, and on this scene the reference's own figure fits inside it
        assert bound[0] <= pc.F16_ALREADY_BOUNDED[cfg.name][0] and bound[1] <= pc.F16_ALREADY_BOUNDED[cfg.name][1]
        assert bound == (worst + 1, 2 * share)
