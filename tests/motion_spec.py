"""NumPy restatement of include/tdk_hip_motion.h: what tdk_motion_pyramid, tdk_motion_match and tdk_motion_temporal_denoise must
compute, to the last bit of the pyramid, the field, the costs, the output, both state planes and the frame index.  The estimator is
integer arithmetic behind one float32 conversion per CFA cell; the filter is tests/temporal_spec.py with the history read at the
displaced site.  Shared by test_motion_spec.py (which holds this file to literal loops and to the block's purpose) and
test_gpu_motion.py (which holds the kernels to this file)."""

import numpy as np

import temporal_spec as tspec

F = np.float32
TILE_W, TILE_H = 64, 32          # sites
BLOCK_W, BLOCK_H = 32, 16        # values of a level
MAX_LEVELS, MAX_SEARCH, MAX_DISPLACEMENT = 4, 4, 78
DEFAULT_LEVELS, DEFAULT_SEARCH, DEFAULT_ZERO_BIAS = 3, 4, 300


def scale_of(white_level=1.0):
    """The float32 the Python side passes: fl32(1 / (4 * white_level))."""
    return F(1.0 / (4.0 * float(F(white_level))))


def max_displacement(levels=DEFAULT_LEVELS, search=DEFAULT_SEARCH):
    return 2 * ((search + 1) * 2 ** (levels - 1) - 1)


def tiles(width, height):
    """(Ty, Tx)"""
    return (-(-height // TILE_H), -(-width // TILE_W))


def level_sizes(width, height, levels):
    """(rows, columns) of every level."""
    out, h, w = [], height // 2, width // 2
    for _ in range(levels):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def level_offsets(width, height, levels):
    """(byte offset of every level in its slot, bytes of a slot)."""
    at, total = [], 0
    for h, w in level_sizes(width, height, levels):
        at.append(total)
        total += tspec.align16(h * w)
    return at, total


def pyramid_bytes(width, height, levels):
    return 2 * level_offsets(width, height, levels)[1]


def grey(frame, scale):
    """Level 0: one uint8 per CFA cell."""
    x = np.asarray(frame).astype(F)
    with np.errstate(all='ignore'):
        q = (x[0::2, 0::2] + x[0::2, 1::2]) + (x[1::2, 0::2] + x[1::2, 1::2])
        u = np.fmin(np.fmax(q * F(scale), F(0.0)), F(1.0))
        return (np.sqrt(u) * F(255.0) + F(0.5)).astype(np.uint8)   # (the value is in 0.5 .. 255.5: the conversion truncates)


def reduce(level):
    """Level k + 1 of level k: (a + b + c + d + 2) >> 2 with the indices clamped to the last row and column."""
    h, w = level.shape
    r0, c0 = np.arange(0, h, 2), np.arange(0, w, 2)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    p = level.astype(np.uint32)
    return ((p[np.ix_(r0, c0)] + p[np.ix_(r0, c1)] + p[np.ix_(r1, c0)] + p[np.ix_(r1, c1)] + 2) >> 2).astype(np.uint8)


def pyramid(frame, scale=None, levels=DEFAULT_LEVELS):
    """The levels 0..K-1 of a mosaic, a list of uint8 planes."""
    out = [grey(frame, scale_of() if scale is None else scale)]
    for _ in range(levels - 1):
        out.append(reduce(out[-1]))
    return out


def pyramid_slot(planes, width, height):
    """The bytes tdk_motion_pyramid writes into a slot: (offset, bytes) per level."""
    at, _ = level_offsets(width, height, len(planes))
    return [(at[k], planes[k].reshape(-1)) for k in range(len(planes))]


def _gather(plane, rows, cols):
    h, w = plane.shape
    return plane[np.ix_(np.clip(rows, 0, h - 1), np.clip(cols, 0, w - 1))].astype(np.int64)


def block_cost(cur, ref, k, ty, tx, dy, dx):
    """cost(d) of tile (ty, tx) at level k."""
    cy, cx = (BLOCK_H * ty + BLOCK_H // 2) >> k, (BLOCK_W * tx + BLOCK_W // 2) >> k
    rows, cols = np.arange(cy - BLOCK_H // 2, cy + BLOCK_H // 2), np.arange(cx - BLOCK_W // 2, cx + BLOCK_W // 2)
    return int(np.abs(_gather(cur, rows, cols) - _gather(ref, rows + dy, cols + dx)).sum())


def key_of(cost, oy, ox):
    return (cost << 14) | ((oy * oy + ox * ox) << 8) | ((oy + 4) << 4) | (ox + 4)


def match_tile(cur, ref, ty, tx, search=DEFAULT_SEARCH, zero_bias=0):
    """((dy, dx) in sites, (cost of the result, cost of zero)) of one tile; cur and ref are lists of levels."""
    levels = len(cur)
    d = (0, 0)
    cost = 0
    for k in range(levels - 1, -1, -1):
        radius = search if k == levels - 1 else 1
        base = (2 * d[0], 2 * d[1]) if k != levels - 1 else (0, 0)
        cy, cx = (BLOCK_H * ty + BLOCK_H // 2) >> k, (BLOCK_W * tx + BLOCK_W // 2) >> k
        rows, cols = np.arange(cy - BLOCK_H // 2, cy + BLOCK_H // 2), np.arange(cx - BLOCK_W // 2, cx + BLOCK_W // 2)
        block = _gather(cur[k], rows, cols)
        # the window of all candidates at once: rows and columns -radius .. BLOCK + radius - 1 around the base
        window = _gather(ref[k], np.arange(rows[0] + base[0] - radius, rows[-1] + base[0] + radius + 1),
                         np.arange(cols[0] + base[1] - radius, cols[-1] + base[1] + radius + 1))
        best = None
        for oy in range(-radius, radius + 1):
            for ox in range(-radius, radius + 1):
                c = int(np.abs(block - window[oy + radius:oy + radius + BLOCK_H, ox + radius:ox + radius + BLOCK_W]).sum())
                key = key_of(c, oy, ox)
                if best is None or key < best[0]:
                    best = (key, oy, ox, c)
        d = (base[0] + best[1], base[1] + best[2])
        cost = best[3]
    zero = block_cost(cur[0], ref[0], 0, ty, tx, 0, 0)
    if cost + zero_bias >= zero:
        d, cost = (0, 0), zero
    return (2 * d[0], 2 * d[1]), (cost, zero)


def match(cur, ref, width, height, search=DEFAULT_SEARCH, zero_bias=0, idx=None):
    """tdk_motion_match: (field (Ty, Tx, 2) int16, costs (Ty, Tx, 2) uint32); idx == 0 (no history) gives zeros."""
    ny, nx = tiles(width, height)
    field, costs = np.zeros((ny, nx, 2), np.int16), np.zeros((ny, nx, 2), np.uint32)
    if idx == 0:
        return field, costs
    for ty in range(ny):
        for tx in range(nx):
            field[ty, tx], costs[ty, tx] = match_tile(cur, ref, ty, tx, search, zero_bias)
    return field, costs


def estimate(cur_frame, ref_frame, levels=DEFAULT_LEVELS, search=DEFAULT_SEARCH, zero_bias=0, white_level=1.0):
    """MotionEstimate.estimate of two mosaics."""
    h, w = np.asarray(cur_frame).shape
    scale = scale_of(white_level)
    return match(pyramid(cur_frame, scale, levels), pyramid(ref_frame, scale, levels), w, h, search, zero_bias)


def displaced(plane, field, fill=0):
    """plane[h] with h = q + (field of q's tile & ~1) for every site q, and which of those h lie inside the frame."""
    h, w = plane.shape
    i, j = np.indices((h, w))
    d = field.astype(np.int64) & ~1
    hi, hj = i + d[i // TILE_H, j // TILE_W, 0], j + d[i // TILE_H, j // TILE_W, 1]
    inside = (hi >= 0) & (hi < h) & (hj >= 0) & (hj < w)
    out = np.full((h, w), fill, plane.dtype)
    out[inside] = plane[hi[inside], hj[inside]]
    return out, inside


def compensated_step(frame, state, field, model, pattern, gains=None, radius=2, thresholds=(1.5, 3.0), pixel_threshold=4.0, max_frames=8.0,
                     variance_floor=1e-12, out_dtype=None):
    """One call of tdk_motion_temporal_denoise: returns `out`, writes the planes idx & 1 of `state` (a temporal_spec.State) and advances
    its index.  The window of an output site evaluates every site q it holds with the OUTPUT tile's displacement, so the e and v of a
    site depend on the tile that asks: the frame is evaluated once per distinct displacement of the field, over the tile and its apron."""
    frame = np.asarray(frame)
    out_dtype = frame.dtype if out_dtype is None else out_dtype
    t_hi, inv, c2, n_max, v_min = tspec.parameters(thresholds, pixel_threshold, max_frames, variance_floor)
    x = frame.astype(F)
    h, w = x.shape
    first = state.idx == 0
    src, dst = (state.idx + 1) & 1, state.idx & 1
    row = tspec.rows_of(x.shape, pattern)
    acc_src, cnt_src = state.acc[src].astype(F), state.cnt[src].astype(F)
    y_all, n_all = np.zeros(x.shape, F), np.zeros(x.shape, F)
    ny, nx = tiles(w, h)
    masked = np.asarray(field).astype(np.int64) & ~1
    cache = {}
    for ty in range(ny):
        for tx in range(nx):
            dy, dx = int(masked[ty, tx, 0]), int(masked[ty, tx, 1])
            if (dy, dx) not in cache:
                A, N = np.zeros(x.shape, F), np.zeros(x.shape, F)
                if not first:
                    uniform = np.broadcast_to(np.array([dy, dx], np.int64), (ny, nx, 2))
                    A, inside = displaced(acc_src, uniform, 0)
                    N, _ = displaced(cnt_src, uniform, 0)
                    A, N = np.where(inside, A, F(0.0)).astype(F), np.where(inside, N, F(0.0)).astype(F)
                d, e, v, valid = tspec.site_terms(x, A, N, model, row, gains, v_min)
                E, V = tspec.window_sums(e, radius), tspec.window_sums(v, radius)
                with np.errstate(all='ignore'):
                    t = E / V
                    s = np.fmin(np.fmax((t_hi - t) * inv, F(0.0)), F(1.0))
                    s = np.where(e > c2 * v, F(0.0), s).astype(F)
                    n1 = np.where(valid, np.fmin(s * N + F(1.0), n_max), F(1.0)).astype(F)
                    y = np.where(n1 == F(1.0), x, A + d / n1).astype(F)
                cache[(dy, dx)] = (y, n1)
            y, n1 = cache[(dy, dx)]
            sl = (slice(TILE_H * ty, TILE_H * (ty + 1)), slice(TILE_W * tx, TILE_W * (tx + 1)))
            y_all[sl], n_all[sl] = y[sl], n1[sl]
    state.acc[dst] = y_all.astype(state.acc[dst].dtype)
    state.cnt[dst] = n_all.astype(np.float16)
    state.idx = tspec.next_index(state.idx)
    return y_all.astype(out_dtype)


class Sequence:
    """MotionTemporalDenoise.process of one key: the state, the two pyramid slots and the last field and costs."""

    def __init__(self, shape, state_dtype=np.float32, levels=DEFAULT_LEVELS, search=DEFAULT_SEARCH, zero_bias=0, white_level=1.0, fill=np.nan):
        self.state = tspec.State(shape, state_dtype, fill=fill)
        self.levels, self.search, self.zero_bias, self.scale = levels, search, zero_bias, scale_of(white_level)
        self.slots = [None, None]
        self.field = self.costs = None

    def step(self, frame, model, pattern, **kw):
        h, w = np.asarray(frame).shape
        idx = self.state.idx
        self.slots[idx & 1] = pyramid(frame, self.scale, self.levels)
        if idx == 0:
            self.field, self.costs = match(None, None, w, h, idx=0)
        else:
            self.field, self.costs = match(self.slots[idx & 1], self.slots[(idx + 1) & 1], w, h, self.search, self.zero_bias)
        return compensated_step(frame, self.state, self.field, model, pattern, **kw)
