"""NumPy restatement of include/tdk_hip_temporal.h: what tdk_temporal_denoise and tdk_temporal_reset must compute, to the last bit of
the output, of both state planes and of the frame index.  float32 operation by operation, one rounding each.  Shared by
test_temporal_spec.py (which holds this file to a second, per-site evaluation and to the algorithm's purpose) and
test_gpu_temporal.py (which holds the kernel to this file)."""

import numpy as np

RGGB, BGGR, GRBG, GBRG = 0x94949494, 0x16161616, 0x61616161, 0x49494949
F = np.float32
HEAD_BYTES = 16


def align16(n):
    return (n + 15) // 16 * 16


def state_bytes(width, height, state_dtype=np.float32):
    """The documented layout: the head, acc[0], acc[1], cnt[0], cnt[1], every plane on a multiple of 16 bytes."""
    return HEAD_BYTES + 2 * align16(width * height * np.dtype(state_dtype).itemsize) + 2 * align16(width * height * 2)


def rows_of(shape, pattern):
    """The model row (colour) of every site of a mosaic."""
    i, j = np.indices(shape)
    return ((pattern >> (2 * (2 * (i & 1) + (j & 1)))) & 3).astype(np.int64)


def next_index(idx):
    return 2 if idx == 0xFFFFFFFF else idx + 1


class State:
    """The state of one sequence: the index word and the two copies of the two planes.  `fill` is what the planes hold before
    anything has been written: nothing may depend on it."""

    def __init__(self, shape, state_dtype=np.float32, fill=np.nan, idx=0):
        self.idx = idx
        self.acc = [np.full(shape, fill, state_dtype) for _ in range(2)]
        self.cnt = [np.full(shape, fill, np.float16) for _ in range(2)]

    def reset(self):
        self.idx = 0

    def next_read(self):
        """(accumulated, count): the planes the next call will read."""
        p = (self.idx + 1) & 1
        return self.acc[p], self.cnt[p]


def parameters(thresholds=(1.5, 3.0), pixel_threshold=4.0, max_frames=8.0, variance_floor=1e-12):
    """(t_hi, inv, c2, n_max, v_min) as the float32 numbers the kernel is given."""
    t_lo, t_hi = F(thresholds[0]), F(thresholds[1])
    inv = F(1.0) / (t_hi - t_lo)
    c2 = F(np.inf) if pixel_threshold is None else F(pixel_threshold) * F(pixel_threshold)
    return t_hi, inv, c2, F(max_frames), F(variance_floor)


def site_terms(x, A, N, model, row, gains, v_min):
    """(d, e, v, valid) of every site."""
    model = np.asarray(model, F)
    g = np.ones(3, F) if gains is None else np.asarray(gains, F)
    with np.errstate(all='ignore'):
        ap = g * model[:, 0]
        bp = (g * g) * model[:, 1]
        valid = (model[:, 2] != 0)[row]
        d = x - A
        var = np.fmax(ap[row] * np.fmax(A, F(0.0)) + bp[row], v_min)
        v = var + var / np.fmax(N, F(1.0))
        e = d * d
    return d, np.where(valid, e, F(0.0)).astype(F), np.where(valid, v, F(0.0)).astype(F), valid


def window_sums(p, r):
    """Row sums over the in-frame columns in ascending order from 0.0f, then the sum of the row sums over the in-frame rows in
    ascending order from 0.0f.  A site outside the frame enters as +0.0f here; no value of p is -0, so that changes no bit
    (tests/test_temporal_spec.py holds this to an evaluation that skips those sites)."""
    h, w = p.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), F)
    pad[r:r + h, r:r + w] = p
    with np.errstate(all='ignore'):
        rows = np.zeros((h + 2 * r, w), F)
        for k in range(2 * r + 1):
            rows = rows + pad[:, k:k + w]
        out = np.zeros((h, w), F)
        for k in range(2 * r + 1):
            out = out + rows[k:k + h, :]
    return out


def step(frame, state, model, pattern, gains=None, radius=2, thresholds=(1.5, 3.0), pixel_threshold=4.0, max_frames=8.0, variance_floor=1e-12,
         out_dtype=None):
    """One call of tdk_temporal_denoise: returns `out`, writes the planes idx & 1 of `state` and advances its index."""
    frame = np.asarray(frame)
    out_dtype = frame.dtype if out_dtype is None else out_dtype
    t_hi, inv, c2, n_max, v_min = parameters(thresholds, pixel_threshold, max_frames, variance_floor)
    x = frame.astype(F)
    first = state.idx == 0
    src, dst = (state.idx + 1) & 1, state.idx & 1
    A = np.zeros(x.shape, F) if first else state.acc[src].astype(F)
    N = np.zeros(x.shape, F) if first else state.cnt[src].astype(F)
    row = rows_of(x.shape, pattern)
    d, e, v, valid = site_terms(x, A, N, model, row, gains, v_min)
    E, V = window_sums(e, radius), window_sums(v, radius)
    with np.errstate(all='ignore'):
        t = E / V
        s = np.fmin(np.fmax((t_hi - t) * inv, F(0.0)), F(1.0))
        s = np.where(e > c2 * v, F(0.0), s).astype(F)
        n1 = np.where(valid, np.fmin(s * N + F(1.0), n_max), F(1.0)).astype(F)
        y = np.where(n1 == F(1.0), x, A + d / n1).astype(F)
        state.acc[dst] = y.astype(state.acc[dst].dtype)
        state.cnt[dst] = n1.astype(np.float16)
        state.idx = next_index(state.idx)
        return y.astype(out_dtype)
