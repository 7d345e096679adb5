"""Re-derives TDK_NOISE_MEDIAN_FACTOR (include/tdk_hip_noise.h): the median of E / (576 s^2) over 8 x 8 blocks of white Gaussian noise
of variance s^2, E the sum of the squares of the 48 horizontal and 48 vertical second differences of a block.  The mean of the same
quantity is 1 (a second difference 2q - q' - q'' has the variance 6 s^2, and 96 * 6 = 576); the median is lower because E is skewed.

  python profiles/noiseprofile_constants.py [blocks] [seed]        default: 4e6 blocks, default_rng(7), NumPy float64

prints the median, the mean and the standard error of the median (from the spread of the medians of 20 equal parts)."""

import sys

import numpy as np


def energies(blocks, rng, chunk=200000):
    out = np.empty(blocks, np.float64)
    for at in range(0, blocks, chunk):
        n = min(chunk, blocks - at)
        q = rng.standard_normal((n, 8, 8))
        h = 2 * q[:, :, 1:7] - q[:, :, 0:6] - q[:, :, 2:8]
        v = 2 * q[:, 1:7, :] - q[:, 0:6, :] - q[:, 2:8, :]
        out[at:at + n] = ((h * h).sum(axis=(1, 2)) + (v * v).sum(axis=(1, 2))) / 576.0
    return out


def median_factor(blocks=4000000, seed=7):
    """(median, mean) of E / (576 s^2)."""
    e = energies(int(blocks), np.random.default_rng(seed))
    return float(np.median(e)), float(e.mean())


if __name__ == '__main__':
    blocks = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4000000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    e = energies(blocks, np.random.default_rng(seed))
    parts = np.median(e[:blocks // 20 * 20].reshape(20, -1), axis=1)
    print(f'blocks {blocks}, default_rng({seed})')
    print(f'median of E / (576 s^2): {np.median(e):.5f}  (standard error about {parts.std(ddof=1) / np.sqrt(20):.1e})')
    print(f'mean   of E / (576 s^2): {e.mean():.5f}')
