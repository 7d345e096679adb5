"""Case tables and input builders of the Wiener geometry sweep (shared by tests/test_wiener_cases.py, which runs without a GPU, and
tests/test_gpu_wiener_geometry.py).  A plain helper module: no fixtures, no tests, nothing built or loaded.

The geometry functions restate, in plain Python, the host code of csrc/wiener.hip (geometry, geometry_ys, pick_segment_rows,
tiles_per_cu, pick_group_width) and the per-workgroup quantities at the top of wiener_ystream (csrc/tdk_wiener_ystream.h), so the
tests can say which branch of a kernel a frame size reaches:

  strip kernel (K = 32, ov = 4): a strip = 16 tile columns = 8 tile pairs, a segment = TR tile rows,
      ntx = (W - 1) // 8 + 4, nty = (H - 1) // 8 + 4, NB = (tile rows of the segment) + 3 blocks of 8 image rows,
      NJ = (NB + 4) // 2 + 2 loop iterations of two blocks each;
  general kernel (the five other (K, ov)): a group = G tile columns x TR = 4 * (64 // K) tile rows, s = K // ov,
      ntx = (W - 1) // s + ov, nty = (H - 1) // s + ov (never below 2 ov - 1: the frame is at least K x K).
"""

import random
from collections import namedtuple

import numpy as np

STRIP_TILES = 16   # ys::NTC
STRIP_TR_MIN = 8   # YS_TR_MIN
GROUP_G_MIN, GROUP_G_MAX = 8, 64
GROUP_PAIRS = [(32, 2), (16, 4), (16, 8), (32, 8), (16, 2)]
SIGMAS = (0.0, 0.02, 0.1, 0.3, 5.0)
SPECTRUM_PAIRS = [(32, 4), (16, 4)]
SPECTRUM_SHAPES = [(73, 101), (97, 233)]  # (h, w)

StripGeom = namedtuple('StripGeom', 'ntx nty TR strips segments last_strip_tiles last_segment_rows NB')
GroupGeom = namedtuple('GroupGeom', 's ntx nty TR G groups_x groups_y last_group_tiles last_group_rows vec')


def div_up(a, b):
    return -(-a // b)


def strip_geometry(W, H, TR=STRIP_TR_MIN):
    """geometry_ys(W, H, TR) and what the last strip / the last segment hold; NB is that of the LAST segment (every other
    segment has TR + 3)."""
    ntx, nty = (W - 1) // 8 + 4, (H - 1) // 8 + 4
    strips, segments = div_up(ntx, STRIP_TILES), div_up(nty, TR)
    last_rows = nty - TR * (segments - 1)
    return StripGeom(ntx, nty, TR, strips, segments, ntx - STRIP_TILES * (strips - 1), last_rows, last_rows + 3)


def strip_blocks(W, H, TR=STRIP_TR_MIN):
    """NB of every segment of a strip, top to bottom."""
    g = strip_geometry(W, H, TR)
    return [min(TR, g.nty - TR * k) + 3 for k in range(g.segments)]


def _strip_slab_floats(W, H, TR):
    g = strip_geometry(W, H, TR)
    rsx = STRIP_TILES * 8 + 32 - 8
    return g.strips * g.segments * ((rsx + 3) & ~3) * (TR * 8 + 32 - 8)


def _group_slab_floats(W, H, K, ov, G):
    g = group_geometry(W, H, K, ov, G)
    rsx = G * g.s + K - g.s
    return g.groups_x * g.groups_y * ((rsx + 3) & ~3) * (g.TR * g.s + K - g.s)


def pick_segment_rows(W, H, nplanes, cus):
    """pick_segment_rows of csrc/wiener.hip: fewest rounds x (TR + 4) steps with 2 workgroups per CU, inside the workspace."""
    cap = max(_group_slab_floats(W, H, 32, 4, GROUP_G_MIN), _strip_slab_floats(W, H, STRIP_TR_MIN))
    slots = 2 * cus
    nty = strip_geometry(W, H).nty
    best, best_cost = STRIP_TR_MIN, 1e30
    for tr in range(STRIP_TR_MIN, max(nty, STRIP_TR_MIN) + 1):
        if _strip_slab_floats(W, H, tr) > cap:
            continue
        g = strip_geometry(W, H, tr)
        rounds = div_up(g.strips * g.segments * nplanes, slots)
        cost = rounds * (tr + 4.0)
        if cost < best_cost - 1e-9:
            best, best_cost = tr, cost
    return best


def strip_groups(W, H, C):
    """Workgroups of the strip kernel's launch with TR = 8."""
    g = strip_geometry(W, H)
    return g.strips * g.segments * C


def group_geometry(W, H, K, ov, G=GROUP_G_MIN):
    s = K // ov
    ntx, nty = (W - 1) // s + ov, (H - 1) // s + ov
    TR = NWV * (64 // K)
    gx, gy = div_up(ntx, G), div_up(nty, TR)
    return GroupGeom(s, ntx, nty, TR, G, gx, gy, ntx - G * (gx - 1), nty - TR * (gy - 1), W % 4 == 0 and s % 4 == 0)


NWV = 4                  # csrc/wiener.hip: waves per workgroup of the general tile kernel (TR = NWV * (64 // K))
WAVES_PER_SIMD = 3       # csrc/wiener.hip: TDK_WIENER_WAVES_PER_SIMD, the kernel's launch bound


def tiles_per_cu(K, ov):
    """tiles_per_cu of csrc/wiener.hip: workgroups per CU by LDS (160 KB) and by waves (4 SIMDs)."""
    s, TR = K // ov, NWV * (64 // K)
    lds = (1 if 2 * s >= 32 else 2) * TR * K * 2 * s * 4
    return min(160 * 1024 // lds, 4 * WAVES_PER_SIMD // NWV)


def pick_group_width(W, H, K, ov, nplanes, cus):
    """pick_group_width of csrc/wiener.hip: the width whose rounds are fullest, inside the workspace of G = 8."""
    slots = cus * tiles_per_cu(K, ov)
    cap = _group_slab_floats(W, H, K, ov, GROUP_G_MIN)
    best, best_eff = GROUP_G_MIN, -1.0
    for G in range(GROUP_G_MIN, GROUP_G_MAX + 1, 2):
        if _group_slab_floats(W, H, K, ov, G) > cap:
            continue
        g = group_geometry(W, H, K, ov, G)
        rounds = div_up(g.groups_x * g.groups_y * nplanes, slots)
        steps = G // 2 + (K - g.s + 2 * g.s - 1) // (2 * g.s)
        eff = (g.ntx / 2 * g.groups_y * nplanes) / (rounds * slots * steps)
        if eff > best_eff + 1e-9:
            best, best_eff = G, eff
    return best


# ---------------------------------------------------------------------------------------------------------------- strip kernel
# (W, H) for (K, ov) = (32, 4).  Names as in wiener_ystream: xa / xb (ya / yb) = tile a / b of a tile pair exists, seen from the
# row stages (the column stage); fa / fb = the factors of the branch taken when a strip has a missing tile; sx_lim = first strip
# sample beyond the strip's last tile; fetch = the 16-B load of an in-frame group of 4 samples (C = 1, W % 4 == 0 only),
# fetch_edge = per-sample reflected loads; NB / NJ as above.  "seam": the three carried blocks a segment leaves for the next one.
# Widths: 32 (ntx 7), 35 (8), 89 (15), 97 / 104 (16), 105 (17), 113 (18), 130 (20), 225 / 232 (32), 233 (33), 361 (49).
# Heights: 32 (nty 7), 33 / 40 (8), 41 (9) ... 97 (16), 105 (17).
STRIP_SHAPES_FIXED = [
    (32, 32),    # smallest frame: every group of 4 touches a frame edge or lies past sx_lim; ntx = 7: pair 3 is xa && !xb (fa / fb), pairs 4-7 absent; nty = 7 < TR, NB = 10
    (32, 41),    # one strip, nty = 9: a second segment of ONE tile row, NB = 4 (the smallest), NJ = 6; seam above it
    (32, 105),   # one half-filled strip, three segments (8, 8, 1): two seams in a strip whose right part is all !xa
    (35, 33),    # W % 4 = 3: fetch_edge for every group (vec off); ntx = 8: four whole pairs, pairs 4-7 absent (!xa && !xb, ya / yb off in waves 2, 3); exactly one segment
    (35, 49),    # nty = 10: last segment of 2 rows, NB = 5 (odd: the loop's last pair of blocks is half empty)
    (35, 89),    # nty = 15: last segment of 7 rows, NB = 10, with W % 4 = 3
    (89, 40),    # ntx = 15: odd count, the last pair is xa && !xb while every other pair is whole; H = 40: largest frame of one full segment (nty = 8, NB = 11)
    (89, 57),    # ntx = 15 with a last segment of 3 rows, NB = 6
    (89, 97),    # ntx = 15 with two full segments (nty = 16): seam between two NB = 11 segments
    (97, 32),    # ntx = 16: exactly one strip, all pairs whole (the ballot branch without fa / fb); W % 4 = 1; nty = 7
    (97, 65),    # one whole strip, last segment of 4 rows, NB = 7 (odd)
    (97, 105),   # one whole strip, three segments
    (104, 33),   # W % 4 = 0: fetch for the in-frame groups, fetch_edge only for the groups left of x = 0 and right of x = W; largest W of one strip
    (104, 41),   # vector fetch with a second segment of one tile row
    (104, 73),   # vector fetch, last segment of 5 rows, NB = 8 (even)
    (105, 40),   # ntx = 17: the second strip holds a single tile (pair 0 is xa && !xb, all else absent), sx_lim = 32 keeps its reads inside one reflection
    (105, 49),   # single-tile last strip with NB = 5 in the last segment
    (105, 81),   # single-tile last strip, last segment of 6 rows, NB = 9 (odd)
    (113, 32),   # ntx = 18: last strip of two tiles = one whole pair, the rest absent (fa = fb = 1 on pair 0 only)
    (113, 57),   # two-tile last strip, last segment of 3 rows
    (113, 89),   # two-tile last strip, last segment of 7 rows, NB = 10
    (130, 33),   # W % 4 = 2 (fetch_edge everywhere), ntx = 20: last strip of four tiles
    (130, 65),   # W % 4 = 2, last segment of 4 rows, NB = 7
    (130, 97),   # W % 4 = 2, two full segments
    (225, 40),   # ntx = 32: exactly two whole strips (no strip takes the fa / fb branch); the x seam between strips in the finish kernels
    (225, 73),   # two whole strips, last segment of 5 rows
    (225, 105),  # two whole strips, three segments
    (232, 41),   # two whole strips with W % 4 = 0 (vector fetch in both), second segment of one row; largest W of two strips
    (232, 81),   # the same with a last segment of 6 rows, NB = 9
    (233, 49),   # ntx = 33: a third strip with one tile, NB = 5
    (233, 89),   # three strips (16, 16, 1), last segment of 7 rows
    (361, 57),   # ntx = 49: four strips, the last with one tile; last segment of 3 rows
    (361, 97),   # four strips, two full segments
    (361, 105),  # four strips x three segments: at least 3 of each, every seam direction at once
]
_rng = random.Random(14)
STRIP_SHAPES_RANDOM = [(_rng.randint(32, 400), _rng.randint(32, 140)) for _ in range(6)]  # 6 seeded draws: W in 32..400, H in 32..140
STRIP_SHAPES = STRIP_SHAPES_FIXED + STRIP_SHAPES_RANDOM

# ---------------------------------------------------------------------------------------------------------------- general kernel
# (W, H) per (K, ov).  Names as in wiener_stream: act_a / act_b = tile a / b of a step exists; row_active = the lane's tile row
# exists; vec_ok = W % 4 == 0 && s % 4 == 0 (16-B row loads where the K + s samples lie inside the frame).  One group = 8 tile
# columns (ntx 8 / 9 / 16 / 17 = one group / + one tile / two groups / + one tile) x TR tile rows (nty TR / TR + 1 / 2 TR + 1
# = one band / + one row / two bands + one row).  ov = 8 frames have ntx, nty >= 15, so ntx 8, 9 (and nty 8, 9 for K = 32) do
# not exist there: those tables take the smallest counts instead.
GROUP_SHAPES = {
    (32, 2): [  # s = 16, TR = 8; 2 s = 32 columns per step (one LDS buffer)
        (32, 32),     # K x K: ntx = nty = 3, one step and a half (act_a && !act_b in step 1), rows 3-7 of the band inactive
        (33, 35),     # (K + 1) x (K + 3): ntx = nty = 4, W % 4 = 1: scalar reflected loads
        (97, 97),     # ntx = 8, nty = 8 = TR: exactly one group, every tile row active; W % 4 = 1
        (112, 113),   # ntx = 8 at its largest W (vec_ok, W % 4 = 0), nty = 9: a second band of one row
        (113, 241),   # ntx = 9: a second group of one tile (act_a && !act_b, then nothing); nty = 17 = 2 TR + 1
        (225, 97),    # ntx = 16: two whole groups, nty = TR
        (240, 113),   # ntx = 16 with vec_ok, nty = TR + 1
        (241, 100),   # ntx = 17: two groups and one tile, W % 4 = 1
        (256, 241),   # ntx = 17 with vec_ok, nty = 2 TR + 1: 3 x 3 groups
    ],
    (16, 4): [  # s = 4, TR = 16
        (16, 16),     # K x K: ntx = nty = 7: act_a && !act_b in step 3, rows 7-15 inactive
        (17, 19),     # (K + 1) x (K + 3): ntx = 8 (one whole group), W % 4 = 1
        (20, 49),     # ntx = 8 with vec_ok (W % 4 = 0), nty = 16 = TR
        (21, 53),     # ntx = 9: second group of one tile; nty = 17 = TR + 1
        (24, 117),    # ntx = 9 with vec_ok, nty = 33 = 2 TR + 1
        (49, 52),     # ntx = 16: two whole groups, nty = TR at its largest H
        (52, 53),     # ntx = 16 with vec_ok, nty = TR + 1
        (53, 49),     # ntx = 17: two groups and one tile, W % 4 = 1
        (56, 117),    # ntx = 17 with vec_ok, nty = 2 TR + 1: 3 x 3 groups
        (50, 117),    # W % 4 = 2, ntx = 16, nty = 2 TR + 1
    ],
    (16, 8): [  # s = 2, TR = 16: vec_ok never holds (s % 4 != 0); ntx, nty >= 15
        (16, 16),     # K x K: ntx = nty = 15: the last step is act_a && !act_b, row 15 inactive
        (17, 19),     # (K + 1) x (K + 3): ntx = 16 (two whole groups), nty = 17 = TR + 1
        (18, 17),     # ntx = 16, nty = 16 = TR: every tile row active; W % 4 = 2
        (19, 17),     # ntx = 17: two groups and one tile, nty = TR; W % 4 = 3
        (20, 19),     # ntx = 17 with W % 4 = 0 (still scalar loads: s = 2), nty = TR + 1
        (18, 51),     # ntx = 16, nty = 33 = 2 TR + 1
        (19, 51),     # ntx = 17, nty = 2 TR + 1: 3 x 3 groups
    ],
    (32, 8): [  # s = 4, TR = 8; ntx, nty >= 15: nty = TR and TR + 1 do not exist, the table takes nty 15, 16 = 2 TR, 17 = 2 TR + 1
        (32, 32),     # K x K: ntx = nty = 15: two groups, the last step act_a && !act_b; last band of 7 rows
        (33, 35),     # (K + 1) x (K + 3): ntx = 16, nty = 16 = 2 TR: two whole groups x two whole bands; W % 4 = 1
        (36, 33),     # ntx = 16 with vec_ok (W % 4 = 0), nty = 2 TR
        (37, 37),     # ntx = 17: two groups and one tile; nty = 17 = 2 TR + 1: 3 x 3 groups; W % 4 = 1
        (40, 37),     # ntx = 17 with vec_ok, nty = 2 TR + 1
        (38, 32),     # W % 4 = 2, ntx = 17, nty = 15
        (36, 37),     # ntx = 16 with vec_ok, nty = 2 TR + 1
    ],
    (16, 2): [  # s = 8, TR = 16
        (16, 16),     # K x K: ntx = nty = 3
        (17, 19),     # (K + 1) x (K + 3): ntx = nty = 4, W % 4 = 1
        (49, 113),    # ntx = 8: one whole group, nty = 16 = TR; W % 4 = 1
        (56, 121),    # ntx = 8 at its largest W with vec_ok, nty = 17 = TR + 1
        (57, 249),    # ntx = 9: second group of one tile; nty = 33 = 2 TR + 1
        (64, 113),    # ntx = 9 with vec_ok, nty = TR
        (113, 121),   # ntx = 16: two whole groups, nty = TR + 1
        (120, 249),   # ntx = 16 with vec_ok, nty = 2 TR + 1
        (121, 113),   # ntx = 17: two groups and one tile, W % 4 = 1
        (126, 249),   # W % 4 = 2, ntx = 17, nty = 2 TR + 1: 3 x 3 groups
    ],
}
# per pair, the shape that also runs float16 and process_log_luminance in the GPU sweep: the 3 x 3 (or largest) grid
GROUP_EXTRA_SHAPE = {(32, 2): (256, 241), (16, 4): (56, 117), (16, 8): (19, 51), (32, 8): (37, 37), (16, 2): (120, 249)}


# ---------------------------------------------------------------------------------------------------------------- inputs
def loglum_plane(scene, oracle, h, w, seed=7, clipped=False):
    """The log-lightness log(max(1e-4, L)) of a synthetic scene, the denoiser's input in the pipeline: possible range
    [log 1e-4, 0] = [-9.21, 0], of which the scene itself fills about [-2, -0.2].  clipped: with a black and a white patch, so
    that both ends of the range occur, next to each other's neighbourhoods (tiles whose samples differ by 9).
    scene, oracle: the fixtures of tests/conftest.py (this module builds and loads nothing itself)."""
    rgb = scene(h, w, seed).copy()
    if clipped:
        rgb[h // 5:h // 5 + 9, w // 4:w // 4 + 13] = 0.0
        rgb[h // 2:h // 2 + 7, w // 2:w // 2 + 11] = 1.0
    return oracle.compute_luminance(rgb, log=True, eps=1e-4)


def bin_patterns(h, w, K):
    """{name: plane} of the single-bin patterns: a cosine of amplitude 0.02 on 0.5 at the tile's Nyquist bin of x, y, both
    (the self-conjugate bins K / 2), and a cosine at bins 1, 5, K / 2 - 1 of each axis (conjugate pairs).  The tile origins are
    multiples of K / ov, so away from the reflected frame edges every tile sees the same bin.  The conjugate-pair cosines have
    amplitude 0.02 for K = 32 and 0.03 for K = 16: a 16 x 16 window collects a quarter of the power, and at 0.02 the bin sits
    at sigma^2 = 0.01 (gain ~ 0, within 1.5e-3 of full removal) instead of being partially attenuated at sigma = 0.1."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    amp = 0.02 if K == 32 else 0.03
    out = {
        'nyq_x': 0.5 + 0.02 * np.cos(np.pi * x),
        'nyq_y': 0.5 + 0.02 * np.cos(np.pi * y),
        'nyq_xy': 0.5 + 0.02 * np.cos(np.pi * x) * np.cos(np.pi * y),
    }
    for k in (1, 5, K // 2 - 1):
        out[f'bin_x{k}'] = 0.5 + amp * np.cos(2 * np.pi * k * x / K)
        out[f'bin_y{k}'] = 0.5 + amp * np.cos(2 * np.pi * k * y / K)
    return {n: v.astype(np.float32) for n, v in out.items()}


def patterns(h, w, K, scene, oracle):
    """{name: float32 (h, w) plane}: inputs on which single spectral bins, single samples and the value range decide the result."""
    rng = np.random.default_rng(1000 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = {'const': np.full((h, w), 0.3, np.float32)}
    out.update(bin_patterns(h, w, K))
    imp = np.full((h, w), 0.2, np.float32)
    imp[0, 0] = imp[h - 1, w - 1] = imp[h // 2, w // 2] = 1.0
    out['impulse'] = imp
    out['ramp'] = (0.1 + 0.6 * x / (w - 1) + 0.3 * y / (h - 1)).astype(np.float32)
    out['noise'] = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    out['faint'] = (0.5 + 0.01 * rng.standard_normal((h, w))).astype(np.float32)
    out['loglum'] = loglum_plane(scene, oracle, h, w)
    return out


def extra_patterns(h, w, scene, oracle):
    """Beyond the plain scene: 'loglum_clip', log-lightness with both ends of [-9.21, 0].  Kept apart from patterns() because its
    values are nine times larger, so every bound on it is stated relative to scale_of()."""
    return {'loglum_clip': loglum_plane(scene, oracle, h, w, clipped=True)}


def scale_of(x):
    """The factor of the float32 bounds: max(1, max |input|)."""
    return max(1.0, float(np.abs(x).max()))
