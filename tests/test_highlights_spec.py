"""CPU-only: the specification of the highlight stage (head comment of include/tdk_hip_highlights.h) as a NumPy restatement,
`highlights_ref`.  Every written operation is one correctly rounded float32 operation in the order of the header, which is what the
kernels are asked to reproduce bit for bit (tests/test_gpu_highlights.py imports this module, and its cases).  It is written from
the text of the specification -- sums and counts per colour over the 3x3 neighbourhood, row-major -- not from the kernel, which
splits the neighbourhood by CFA position; `highlights_loop`, a plain loop over the sites, is a second restatement it is held
against on the small frames.

Also asserted here: what the GPU cases rely on, so that none of them passes on an empty case."""
import numpy as np
import pytest

F = np.float32
PATTERNS = {'RGGB': 0x94949494, 'BGGR': 0x16161616, 'GRBG': 0x61616161, 'GBRG': 0x49494949}
TILE = (128, 16)   # (width, height) of a workgroup's tile: torch_darktable.Highlights.TILE
SCALE = F(1048576.0)
GAINS = {'daylight': (1.9, 1.0, 1.6), 'green_largest': (0.8, 1.3, 0.9)}


def colour_map(h, w, pattern):
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    p = 2 * (i & 1) + (j & 1)
    return ((pattern >> (2 * p)) & 3).astype(np.int64)


def reference_values(v, col):
    """ref(i, j): S_k and n_k over the 3x3 neighbourhood, sites visited row-major, missing sites skipped."""
    h, w = v.shape
    m = np.zeros((h + 2, w + 2), dtype=F)
    m[1:-1, 1:-1] = np.fmax(v, F(0))
    cc = np.full((h + 2, w + 2), -1, dtype=np.int64)
    cc[1:-1, 1:-1] = col
    S, n = np.zeros((3, h, w), dtype=F), np.zeros((3, h, w), dtype=np.int64)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            x, c = m[1 + di:1 + di + h, 1 + dj:1 + dj + w], cc[1 + di:1 + di + h, 1 + dj:1 + dj + w]
            for k in range(3):
                S[k] = np.where(c == k, S[k] + x, S[k])
                n[k] += c == k
    assert n.min() >= 1
    mean = S / n.astype(F)
    a = np.where(col == 0, 1, 0)          # the two colours other than c, a < b
    b = np.where(col == 2, 1, 2)
    pick = lambda k: np.take_along_axis(mean, k[None], axis=0)[0]   # noqa: E731
    return F(0.5) * (pick(a) + pick(b))


def near_clipped(clipped):
    h, w = clipped.shape
    pad = np.zeros((h + 4, w + 4), dtype=bool)
    pad[2:-2, 2:-2] = clipped
    out = np.zeros((h, w), dtype=bool)
    for di in range(5):
        for dj in range(5):
            out |= pad[di:di + h, dj:dj + w]
    return out


def highlights_ref(L, gains, pattern, mode='opposed', threshold=0.98, low=0.2, min_count=64, out_dtype=np.float32, chroma=None, details=False):
    """L: (H, W) float32 or float16.  Returns (out as out_dtype, sum int64[3], cnt int64[3], chroma float32[3])."""
    L = np.asarray(L).astype(F)
    h, w = L.shape
    assert h % 2 == 0 and w % 2 == 0
    g, t, lo = np.asarray(gains, dtype=F), F(threshold), F(low)
    col = colour_map(h, w, pattern)
    with np.errstate(invalid='ignore', over='ignore'):
        v = L * g[col]
        clipped = L >= t
        cl = t * g
        if mode == 'clip':
            m = np.fmin(np.fmin(cl[0], cl[1]), cl[2])
            return np.fmin(np.fmax(v, F(0)), m).astype(out_dtype), None, None, None
        assert mode == 'opposed'
        ref = reference_values(v, col)
        d = v - ref
        contributes = ~clipped & (v > (lo * cl)[col]) & near_clipped(clipped) & (np.abs(d) <= F(64))
        q = np.rint(np.where(contributes, d, F(0)) * SCALE).astype(np.int64)
        total = np.array([q[contributes & (col == k)].sum() for k in range(3)], dtype=np.int64)
        cnt = np.array([(contributes & (col == k)).sum() for k in range(3)], dtype=np.int64)
        if chroma is None:
            chroma = np.array([F(np.float64(total[k]) / (np.float64(cnt[k]) * 1048576.0)) if cnt[k] >= min_count else F(0) for k in range(3)], dtype=F)
        else:
            chroma = np.asarray(chroma, dtype=F)
        out = np.where(clipped, np.fmax(v, ref + chroma[col]), np.fmax(v, F(0))).astype(out_dtype)
    if details:
        return out, total, cnt, chroma, dict(clipped=clipped, contributes=contributes, d=d, ref=ref, v=v)
    return out, total, cnt, chroma


def highlights_loop(L, gains, pattern, threshold=0.98, low=0.2, min_count=64):
    """The same in a plain loop over the sites, float32 scalars: (out float32, sum, cnt, chroma)."""
    L = np.asarray(L).astype(F)
    h, w = L.shape
    g, t, lo = [F(x) for x in gains], F(threshold), F(low)
    colour = lambda i, j: (pattern >> (2 * (2 * (i & 1) + (j & 1)))) & 3   # noqa: E731
    fmax = lambda a, b: b if np.isnan(a) else (a if np.isnan(b) else max(a, b))   # noqa: E731
    inside = lambda i, j: 0 <= i < h and 0 <= j < w   # noqa: E731
    v = np.array([[L[i, j] * g[colour(i, j)] for j in range(w)] for i in range(h)], dtype=F)
    clipped = np.array([[bool(L[i, j] >= t) for j in range(w)] for i in range(h)])
    ref = np.zeros((h, w), dtype=F)
    total, cnt = [0, 0, 0], [0, 0, 0]
    for i in range(h):
        for j in range(w):
            S, n = [F(0), F(0), F(0)], [0, 0, 0]
            for ii in (i - 1, i, i + 1):
                for jj in (j - 1, j, j + 1):
                    if inside(ii, jj):
                        k = colour(ii, jj)
                        S[k] = F(S[k] + fmax(v[ii, jj], F(0)))
                        n[k] += 1
            a, b = [k for k in range(3) if k != colour(i, j)]
            ref[i, j] = F(F(0.5) * F(F(S[a] / F(n[a])) + F(S[b] / F(n[b]))))
    for i in range(h):
        for j in range(w):
            c = colour(i, j)
            near = any(clipped[ii, jj] for ii in range(i - 2, i + 3) for jj in range(j - 2, j + 3) if inside(ii, jj))
            d = F(v[i, j] - ref[i, j])
            if not clipped[i, j] and v[i, j] > F(lo * F(t * g[c])) and near and abs(d) <= F(64):
                total[c] += int(np.rint(F(d * SCALE)))
                cnt[c] += 1
    chroma = [F(np.float64(total[k]) / (np.float64(cnt[k]) * 1048576.0)) if cnt[k] >= min_count else F(0) for k in range(3)]
    out = np.zeros((h, w), dtype=F)
    for i in range(h):
        for j in range(w):
            out[i, j] = fmax(v[i, j], F(ref[i, j] + chroma[colour(i, j)])) if clipped[i, j] else fmax(v[i, j], F(0))
    return out, np.array(total, dtype=np.int64), np.array(cnt, dtype=np.int64), np.array(chroma, dtype=F)


# ------------------------------------------------------------------ the cases (shared with tests/test_gpu_highlights.py)
def scene(h, w, seed, blobs=(), peak=0.85):
    """A smooth linear mosaic below `peak` with a little noise, and blobs (row, column, radius) that run into the sensor's
    saturation at 1.0: a plateau of clipped sites with a rim of bright unclipped ones."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    base = 0.5 + 0.2 * np.sin(i / 7.0 + seed) * np.cos(j / 11.0) + 0.1 * rng.random((h, w))
    base = base * (peak / 0.8)
    for ci, cj, r in blobs:
        base = base + 0.9 * np.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2.0 * r * r))
    return np.minimum(base, 1.0).astype(F)


def plant(L, sites, value=1.0):
    L = L.copy()
    for i, j in sites:
        L[i, j] = value
    return L


def seam_sites(h, w):
    """A clipped site in each frame corner, on each frame edge and on both sides of a tile seam in each direction (needs a frame of
    more than one tile both ways)."""
    tw, th = TILE
    assert w > tw + 1 and h > th + 1
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 70), (h - 1, 90), (12, 0), (20, w - 1),
            (5, tw - 1), (5, tw), (th - 1, 40), (th, 40)] + ([(20, 2 * tw - 1), (20, 2 * tw)] if w > 2 * tw else []) + (
                [(2 * th - 1, 150), (2 * th, 150)] if h > 2 * th else [])


def cases():
    """{name: (L float32 (H, W), keyword arguments of highlights_ref)}.  Sizes (W x H): 2x2, 4x6, 130x18, 258x34, 200x50; the two
    middle ones are one and two tiles plus two sites in each direction."""
    tw, th = TILE
    out = {}
    out['2x2'] = (np.array([[1.0, 0.5], [0.6, 0.99]], dtype=F), dict(min_count=1))
    out['4x6'] = (plant(scene(6, 4, 1), [(0, 0), (3, 2), (5, 3)]), dict(min_count=1))
    one = scene(th + 2, tw + 2, 2, blobs=[(6, 30, 4.0), (th, tw - 2, 3.0)])
    one = plant(plant(plant(one, [(0, 0), (th + 1, tw + 1), (th - 1, 64), (th, 64), (3, tw - 1), (3, tw)]), [(7, 27), (2, 90)], np.nan), [(8, 36), (10, 100)], -0.25)
    out['130x18'] = (one, dict(min_count=8))
    two = scene(2 * th + 2, 2 * tw + 2, 3, blobs=[(10, 50, 6.0), (25, 180, 5.0), (th, tw, 4.0)])
    out['258x34'] = (plant(two, seam_sites(2 * th + 2, 2 * tw + 2)), dict())
    odd = plant(plant(plant(scene(50, 200, 4), [(20, 100), (20, 101), (21, 100)]), [(19, 99)], np.nan), [(22, 102), (40, 7)], -0.5)
    out['200x50'] = (odd, dict())
    out['low0'] = (out['130x18'][0], dict(min_count=8, low=0.0))
    out['none'] = (scene(2 * th + 2, 2 * tw + 2, 5), dict())
    return out


CASES = cases()


def bits(x):
    return np.ascontiguousarray(x).view({2: np.int16, 4: np.int32}[x.dtype.itemsize])


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize('pattern', sorted(PATTERNS))
@pytest.mark.parametrize('name', ['2x2', '4x6', '130x18', 'low0'])
def test_restatement_equals_the_plain_loop(name, pattern):
    L, kw = CASES[name]
    for gains in GAINS.values():
        out, total, cnt, chroma = highlights_ref(L, gains, PATTERNS[pattern], **kw)
        out2, total2, cnt2, chroma2 = highlights_loop(L, gains, PATTERNS[pattern], **kw)
        assert total.tolist() == total2.tolist() and cnt.tolist() == cnt2.tolist()
        assert np.array_equal(bits(chroma), bits(chroma2)) and np.array_equal(bits(out), bits(out2))


def test_the_cases_are_not_empty():
    """What the GPU tests rely on."""
    tw, th = TILE
    sizes = {name: L.shape[::-1] for name, (L, _) in CASES.items()}
    assert [sizes[n] for n in ('2x2', '4x6', '130x18', '258x34', '200x50')] == [(2, 2), (4, 6), (tw + 2, th + 2), (2 * tw + 2, 2 * th + 2), (200, 50)]
    signs = set()
    for pattern in PATTERNS.values():
        for gains in GAINS.values():
            # every colour reaches min_count (the default, 64) in the two-tile frame, and both signs of d contribute
            L, kw = CASES['258x34']
            out, total, cnt, chroma, x = highlights_ref(L, gains, pattern, details=True, **kw)
            assert cnt.min() >= 64 and np.all(chroma != 0), (cnt, chroma)
            d = x['d'][x['contributes']]
            assert (d < 0).any() and (d > 0).any()
            signs |= set(np.sign(chroma).tolist())
            assert x['clipped'].sum() > 100 and (out[x['clipped']] > 1.0).any()          # not clamped from above
            v = L * np.asarray(gains, dtype=F)[colour_map(*L.shape, pattern)]
            assert (bits(out) != bits(np.fmax(v, F(0)))).sum() > 50                      # sites really are rebuilt
            # some colour stays below min_count where three sites are clipped
            L, kw = CASES['200x50']
            _, _, cnt, chroma = highlights_ref(L, gains, pattern, **kw)
            assert 0 < cnt.max() < 64 and np.all(chroma == 0), cnt
            # low = 0 admits sites that low = 0.2 leaves out? at least it never loses one, and negative sites never contribute
            L, kw = CASES['130x18']
            _, _, cnt_low, _ = highlights_ref(L, gains, pattern, **CASES['low0'][1])
            _, _, cnt_def, _, x = highlights_ref(L, gains, pattern, details=True, **kw)
            assert np.all(cnt_low >= cnt_def) and cnt_def.min() >= 8
            assert np.isnan(L).sum() == 2 and (L < 0).sum() == 2 and not x['contributes'][np.isnan(L) | (L < 0)].any()
            assert near_clipped(x['clipped'])[np.isnan(L)].any()                          # a NaN site sits next to clipped ones
    assert signs == {-1.0, 1.0}
    # no clipped site at all
    L, _ = CASES['none']
    assert L.max() < F(0.98)
    # a clipped site in each corner, on each edge and on both sides of a tile seam
    L, _ = CASES['258x34']
    c = L >= F(0.98)
    h, w = L.shape
    assert c[0, 0] and c[0, -1] and c[-1, 0] and c[-1, -1]
    assert c[0, 1:-1].any() and c[-1, 1:-1].any() and c[1:-1, 0].any() and c[1:-1, -1].any()
    for s in (tw, 2 * tw):
        assert (c[:, s - 1] & c[:, s]).any(), s
    for s in (th, 2 * th):
        assert (c[s - 1, :] & c[s, :]).any(), s


@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_identities(pattern):
    """No clipped site: fmaxf(L * g[c], 0), and where v <= 1 the bits of the plain white balance (multiply, clamp to [0, 1])."""
    L, kw = CASES['none']
    L = plant(L, [(3, 3), (9, 200)], -0.3)
    for gains in GAINS.values():
        g = np.asarray(gains, dtype=F)[colour_map(*L.shape, PATTERNS[pattern])]
        out, total, cnt, chroma = highlights_ref(L, gains, PATTERNS[pattern], **kw)
        assert total.tolist() == [0, 0, 0] and cnt.tolist() == [0, 0, 0] and chroma.tolist() == [0, 0, 0]
        assert np.array_equal(bits(out), bits(np.fmax(L * g, F(0))))
        wb = np.fmin(np.fmax(L * g, F(0)), F(1))
        assert (out > 1).any() and np.array_equal(bits(out)[out <= 1], bits(wb)[out <= 1])


def test_clip_mode_and_supplied_chrominance():
    L, kw = CASES['258x34']
    gains = GAINS['daylight']
    out, _, _, _ = highlights_ref(L, gains, PATTERNS['RGGB'], mode='clip')
    m = F(F(0.98) * F(1.0))
    assert out.max() == m and out.min() >= 0
    g = np.asarray(gains, dtype=F)[colour_map(*L.shape, PATTERNS['RGGB'])]
    assert np.array_equal(out, np.minimum(np.maximum(L * g, 0), m))
    a = highlights_ref(L, gains, PATTERNS['RGGB'], **kw)
    b = highlights_ref(L, gains, PATTERNS['RGGB'], chroma=a[3], min_count=10 ** 9)   # used as they are: min_count is not applied again
    assert np.array_equal(bits(a[0]), bits(b[0]))
    c = highlights_ref(L, gains, PATTERNS['RGGB'], chroma=(0.5, -0.25, 0.125))
    assert not np.array_equal(bits(a[0]), bits(c[0]))


def test_binary16_frames_round_once_at_the_store():
    L, kw = CASES['258x34']
    half = L.astype(np.float16)
    out32, total, cnt, chroma = highlights_ref(half, GAINS['daylight'], PATTERNS['GRBG'], **kw)
    out16, total16, cnt16, _ = highlights_ref(half, GAINS['daylight'], PATTERNS['GRBG'], out_dtype=np.float16, **kw)
    assert out16.dtype == np.float16 and np.array_equal(bits(out16), bits(out32.astype(np.float16)))
    assert total.tolist() == total16.tolist() and cnt.tolist() == cnt16.tolist() and cnt.min() >= 64
