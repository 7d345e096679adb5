"""CPU-only: a float64 restatement of the local Laplacian filter with explicit binary16 rounding at every store
(tests/laplacian_spec.py), against the C oracle (fp32 arithmetic, binary16 storage).

Written from the reference's formulas (csrc/local_contrast/laplacian.cu:50-66 sizes and boundary clamp, :111-141 expand,
:177-207 reduce, :221-252 assemble, :266-290 curve, :482-592 sequencing) as whole-array numpy
operations: coordinate arrays and gathers instead of per-pixel loops, float64 instead of float32.  The two restatements
share no code; they can differ only where the oracle's fp32 rounding moves a value across a binary16 rounding boundary,
i.e. by one binary16 ulp of the stored value, on a small share of the pixels -- which is what the test allows."""

import numpy as np
import pytest

from laplacian_spec import half_ulp_of, laplacian_fp64


@pytest.mark.parametrize('size', [(40, 56), (33, 47), (64, 64)])
@pytest.mark.parametrize('params', [(0.2, 1.0, 1.0, 0.0), (0.2, 1.6, 0.7, 0.3), (0.1, 0.5, 1.5, -0.2)])
def test_laplacian_fp64_restatement_matches_the_oracle_to_one_half_ulp(oracle, scene, size, params):
    h, w = size
    lum = oracle.compute_luminance(scene(h, w, 17 + w))
    ref = oracle.laplacian(lum, *params).astype(np.float64)
    got = laplacian_fp64(lum, *params)
    d = np.abs(got - ref)
    # both are binary16-valued; they may sit on neighbouring binary16 values where fp32 vs fp64 rounding differs
    assert (d <= half_ulp_of(np.maximum(np.abs(got), np.abs(ref))) * 1.0001).all(), f'max {d.max():.3e}'
    assert (d > 0).mean() < 2e-3, f'{(d > 0).mean():.4f} of the pixels differ'  # measured: 0 to 4.5e-4


def test_laplacian_identity_settings(oracle, scene):
    """shadows = highlights = 1, clarity = 0: the curve is the identity, the filter returns the binary16-rounded input
    up to the storage rounding of the pyramid (SURVEY.md 8c identity 6)."""
    lum = oracle.compute_luminance(scene(48, 48, 3))
    got = laplacian_fp64(lum, 0.2, 1.0, 1.0, 0.0)
    assert np.abs(got - lum).max() < 2e-3
