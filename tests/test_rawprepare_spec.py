"""CPU-only: the specification of the raw stage (head comment of include/tdk_hip_raw.h) as a NumPy restatement, `raw_prepare_ref`.
With dtype float32 every written operation is one correctly rounded float32 operation in the order of the header, which is what the
kernel is asked to reproduce bit for bit (tests/test_gpu_rawprepare.py imports this module); with dtype float64 it is the plain
version the float32 one is held against here.

Also pinned: the identity is `code / 4095` in float32, grid nodes are hit exactly on their pixels, and what the defect rules do to
planted hot and dead sites, to a ramp, to two hot sites next to each other and to a corner."""
import numpy as np

PATTERNS = {'RGGB': 0x94949494, 'BGGR': 0x16161616, 'GRBG': 0x61616161, 'GBRG': 0x49494949}


def colours(pattern):
    """Colour (0 R, 1 G, 2 B) of the four CFA positions p = 2*(i & 1) + (j & 1)."""
    return np.array([(pattern >> (2 * p)) & 3 for p in range(4)])


def position_map(h, w):
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return 2 * (i & 1) + (j & 1)


def pack12(codes, ids):
    """(H, W) codes 0..4095 -> flat uint8, three bytes per pixel pair: the inverse of the DECODER's nibble order in both formats
    (csrc/codec.hip: for IDS the decoder takes p0's low nibble from the low half of the third byte)."""
    c = np.asarray(codes, dtype=np.uint32).reshape(-1, 2)
    p0, p1 = c[:, 0], c[:, 1]
    if ids:
        b = np.stack([p0 >> 4, p1 >> 4, ((p1 & 15) << 4) | (p0 & 15)], axis=1)
    else:
        b = np.stack([p0 & 255, ((p1 & 15) << 4) | (p0 >> 8), p1 >> 4], axis=1)
    return b.astype(np.uint8).reshape(-1)


def unpack12(data, ids, h, w):
    b = np.asarray(data, dtype=np.uint32).reshape(-1, 3)
    if ids:
        p0, p1 = (b[:, 0] << 4) | (b[:, 2] & 15), (b[:, 1] << 4) | (b[:, 2] >> 4)
    else:
        p0, p1 = ((b[:, 1] & 15) << 8) | b[:, 0], (b[:, 2] << 4) | (b[:, 1] >> 4)
    return np.stack([p0, p1], axis=1).reshape(h, w)


def scale_of(black, white):
    """black[4], scale[4] as the Python front end forms them: float64 on the host, rounded once."""
    b = np.broadcast_to(np.asarray(black, dtype=np.float64).reshape(-1), (4,))
    return b.astype(np.float32), (1.0 / (float(white) - b)).astype(np.float32)


def _axis(n, g, F):
    pos = np.arange(n, dtype=np.int64)
    t = pos * (g - 1)
    q, r = t // (n - 1), t % (n - 1)
    return q, np.minimum(q + 1, g - 1), r.astype(F) / F(n - 1)


def raw_prepare_ref(raw, pattern, black, scale, hot=False, dead=False, threshold=0.02, ratio=0.5, min_count=3, shading=None, gains=None,
                    clip=False, out_dtype=np.float32, dtype=np.float32):
    """raw: (H, W), the codes or stored floats (converted exactly to `dtype`).  Returns (result as out_dtype, mask uint8)."""
    F = dtype
    raw = np.asarray(raw).astype(F)
    h, w = raw.shape
    p = position_map(h, w)
    black, scale = np.asarray(black, dtype=np.float32).astype(F), np.asarray(scale, dtype=np.float32).astype(F)
    with np.errstate(invalid='ignore', over='ignore'):
        L = (raw - black[p]) * scale[p]
        v, mask = L.copy(), np.zeros((h, w), dtype=np.uint8)
        if hot or dead:
            pad = np.full((h + 4, w + 4), np.nan, dtype=F)
            pad[2:-2, 2:-2] = L
            around = [pad[0:h, 2:w + 2], pad[4:h + 4, 2:w + 2], pad[2:h + 2, 0:w], pad[2:h + 2, 4:w + 4]]   # up, down, left, right
            thr, rat = F(np.float32(threshold)), F(np.float32(ratio))
            if hot:
                lim = L * rat
                count, best = np.zeros((h, w), dtype=np.int32), np.zeros((h, w), dtype=F)
                for n in around:
                    member = n < lim
                    best = np.where(member & ((count == 0) | (n > best)), n, best)
                    count += member
                fire = (L > thr) & (count >= min_count)
                v, mask = np.where(fire, best, v), np.where(fire, np.uint8(1), mask)
            if dead:
                count, best = np.zeros((h, w), dtype=np.int32), np.zeros((h, w), dtype=F)
                for n in around:
                    member = (n > thr) & (L < n * rat)
                    best = np.where(member & ((count == 0) | (n < best)), n, best)
                    count += member
                fire = (mask == 0) & (count >= min_count)
                v, mask = np.where(fire, best, v), np.where(fire, np.uint8(2), mask)
        if shading is not None:
            G = np.asarray(shading, dtype=np.float32).astype(F)
            gh, gw = G.shape[:2]
            qx, qx1, ax = _axis(w, gw, F)
            qy, qy1, ay = _axis(h, gh, F)
            qx, qx1, ax, qy, qy1, ay = qx[None, :], qx1[None, :], ax[None, :], qy[:, None], qy1[:, None], ay[:, None]
            bx, by = F(1) - ax, F(1) - ay
            g0 = G[qy, qx, p] * bx + G[qy, qx1, p] * ax
            g1 = G[qy1, qx, p] * bx + G[qy1, qx1, p] * ax
            g = g0 * by + g1 * ay
            v = v * g
        if gains is not None:
            gain = np.asarray(gains, dtype=np.float32).astype(F)[colours(pattern)[p]]
            v = np.fmin(np.fmax(v * gain, F(0)), F(1))
        elif clip:
            v = np.fmin(np.fmax(v, F(0)), F(1))
        return v.astype(out_dtype), mask


def smooth_field(h, w, seed, noise=0.01):
    """A smooth field in [0.1, 0.3] with a little noise, as float32 L values: dark enough that a site near 1 has every neighbour
    below half its value, bright enough that a site near 0 lies below half of every neighbour."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    f = 0.2 + 0.08 * np.sin(i / 9.0) * np.cos(j / 13.0) + rng.normal(0.0, noise, (h, w))
    return np.clip(f, 0.1, 0.3).astype(np.float32)


UNIT = (np.zeros(4, np.float32), np.ones(4, np.float32))   # black = 0, scale = 1: float input already in L units


# ------------------------------------------------------------------ tests
def test_float32_restatement_agrees_with_float64():
    """Linearise, shade, balance: about eleven float32 roundings of half an ulp each on a value formed without cancellation (codes
    above the black levels, positive gains), so 8 float32 ulps bound the difference to the float64 version with room."""
    rng = np.random.default_rng(1)
    h, w = 46, 70
    codes = rng.integers(300, 4096, (h, w))
    black, scale = scale_of([240.0, 256.0, 250.0, 260.0], 4095.0)
    shading = (1.0 + rng.random((9, 17, 4))).astype(np.float32)
    gains = np.array([1.9, 1.0, 1.6], dtype=np.float32)
    for pattern in PATTERNS.values():
        a, _ = raw_prepare_ref(codes, pattern, black, scale, shading=shading, gains=gains)
        b, _ = raw_prepare_ref(codes, pattern, black, scale, shading=shading, gains=gains, dtype=np.float64, out_dtype=np.float64)
        rel = np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b), 1e-30)
        print(f'float32 vs float64: largest relative difference {rel.max():.3e} = {rel.max() * 2 ** 23:.2f} ulp')
        assert rel.max() <= 8 * 2.0 ** -23
        assert (a < 1).any() and (a == 1).any()   # the clamp is exercised and is not everything
    # the defect decisions are the same in both precisions on a field with planted outliers, and the values agree
    L = smooth_field(h, w, 2)
    L[10, 12], L[31, 40] = 0.99, 0.001
    a, ma = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True, dead=True)
    b, mb = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True, dead=True, dtype=np.float64, out_dtype=np.float64)
    assert np.array_equal(ma, mb) and np.allclose(a, b, rtol=2.0 ** -22, atol=0)


def test_identity_is_code_over_4095_in_float32():
    black, scale = scale_of(0.0, 4095.0)
    assert np.all(black == 0) and np.all(scale == np.float32(1.0) / np.float32(4095.0))
    codes = np.arange(4096).reshape(64, 64)
    for ids in (False, True):
        assert np.array_equal(unpack12(pack12(codes, ids), ids, 64, 64), codes)
    out, mask = raw_prepare_ref(codes, PATTERNS['GRBG'], black, scale)
    want = codes.astype(np.float32) * (np.float32(1.0) / np.float32(4095.0))
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), want.view(np.uint32)) and not mask.any()


def test_grid_nodes_are_hit_exactly_on_their_pixels():
    h, w, gh, gw = 22, 34, 4, 4                      # 33 = 3 * 11, 21 = 3 * 7: nodes on pixels 0, 11, 22, 33 and 0, 7, 14, 21
    rng = np.random.default_rng(3)
    G = (0.5 + rng.random((gh, gw, 4))).astype(np.float32)
    out, _ = raw_prepare_ref(np.ones((h, w), np.float32), PATTERNS['RGGB'], *UNIT, shading=G)
    p = position_map(h, w)
    for ny in range(gh):
        for nx in range(gw):
            i, j = ny * 7, nx * 11
            assert out[i, j] == G[ny, nx, p[i, j]], (ny, nx)
    # between two nodes the gain lies between theirs
    assert min(G[0, 0, 1], G[0, 1, 1]) <= out[0, 5] <= max(G[0, 0, 1], G[0, 1, 1])


def test_planted_hot_and_dead_sites_are_replaced():
    L = smooth_field(48, 64, 4)
    clean = L.copy()
    L[20, 30], L[21, 41] = 0.98, 0.002
    out, mask = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True, dead=True)
    assert mask[20, 30] == 1 and mask[21, 41] == 2 and mask.sum() == 3
    assert out[20, 30] == max(clean[18, 30], clean[22, 30], clean[20, 28], clean[20, 32])
    assert out[21, 41] == min(clean[19, 41], clean[23, 41], clean[21, 39], clean[21, 43])
    untouched = mask == 0
    assert np.array_equal(out[untouched], L[untouched])
    # one rule at a time
    _, hot_only = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True)
    _, dead_only = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, dead=True)
    assert hot_only[20, 30] == 1 and hot_only.sum() == 1 and dead_only[21, 41] == 2 and dead_only.sum() == 2


def test_a_noise_free_ramp_is_untouched_at_ratio_one_half():
    i, j = np.meshgrid(np.arange(40), np.arange(56), indexing='ij')
    L = (0.05 + 0.012 * j + 0.004 * i).astype(np.float32)
    out, mask = raw_prepare_ref(L, PATTERNS['BGGR'], *UNIT, hot=True, dead=True, ratio=0.5)
    assert not mask.any() and np.array_equal(out, L)


def test_two_adjacent_hot_sites_need_min_count_three():
    L = smooth_field(32, 40, 5)
    L[12, 16] = L[12, 18] = 0.97     # same colour, two apart: each sees three ordinary neighbours and the other hot one
    _, m4 = raw_prepare_ref(L, PATTERNS['GBRG'], *UNIT, hot=True, min_count=4)
    out, m3 = raw_prepare_ref(L, PATTERNS['GBRG'], *UNIT, hot=True, min_count=3)
    assert m4[12, 16] == 0 and m4[12, 18] == 0
    assert m3[12, 16] == 1 and m3[12, 18] == 1 and out[12, 16] <= 0.3 and out[12, 18] <= 0.3


def test_a_corner_site_is_never_corrected_at_min_count_three():
    L = smooth_field(32, 40, 6)
    for i, j in ((0, 0), (0, 39), (31, 0), (31, 39), (1, 1), (30, 38)):
        L[i, j] = 0.99
    L[0, 20] = 0.99   # an edge site has three neighbours
    out, mask = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True, dead=True, min_count=3)
    for i, j in ((0, 0), (0, 39), (31, 0), (31, 39), (1, 1), (30, 38)):
        assert mask[i, j] == 0 and out[i, j] == L[i, j], (i, j)
    assert mask[0, 20] == 1
    _, m2 = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True, min_count=2)
    assert m2[0, 0] == 1 and m2[31, 39] == 1


def test_nan_is_never_corrected_and_never_counts():
    L = smooth_field(32, 40, 7)
    L[10, 10] = np.nan
    L[10, 12] = 0.99          # its left neighbour is the NaN: three members are left
    out, mask = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True, dead=True, min_count=4)
    assert mask[10, 10] == 0 and np.isnan(out[10, 10]) and mask[10, 12] == 0
    _, mask = raw_prepare_ref(L, PATTERNS['RGGB'], *UNIT, hot=True, dead=True, min_count=3)
    assert mask[10, 10] == 0 and mask[10, 12] == 1
