"""NumPy restatement of include/tdk_hip_hdralign.h: what tdk_hdralign_pyramid, the matches of a bracket and tdk_hdralign_merge must
compute, to the last bit of the output, the last byte of the mask and of the pyramids and the last integer of the fields and costs.
The pyramid is tests/motion_spec.py with the scale the device computes, the match is that file's, and the merge is
tests/hdrmerge_spec.py of the frames displaced with NaN fill, evaluated once per distinct tuple of displacements and taken tile by tile,
with rule 5 applied behind it.  Shared by test_hdralign_spec.py (which holds this file to literal per-site loops and to the block's
purpose) and test_gpu_hdralign.py (which holds the kernels to this file)."""

import numpy as np

import hdrmerge_spec as hspec
import motion_spec as mspec

F = np.float32
TILE_W, TILE_H = mspec.TILE_W, mspec.TILE_H   # of a displacement: 64 x 32 sites
DEFAULT_ZERO_BIAS = 750                        # of torch_darktable.hdralign


def lds_bytes(r):
    """The merge's and 64 bytes of per-frame displacements."""
    return hspec.lds_bytes(r) + 64


def longest(exposures):
    """hi of tdk_hip_hdr.h: the largest exposure, the lowest such index."""
    e = np.asarray(exposures, F)
    hi = 0
    for f in range(1, e.size):
        if e[f] > e[hi]:
            hi = f
    return hi


def scale_of(scale, exposures, frame):
    """s = scale * (e_hi / exposures[frame]): a float32 division, then a float32 product."""
    e = np.asarray(exposures, F)
    with np.errstate(all='ignore'):
        return F(scale) * (e[longest(e)] / e[frame])


def pyramid(frame, exposures, f, scale=None, levels=mspec.DEFAULT_LEVELS):
    """tdk_hdralign_pyramid of frame f of a bracket: the levels, a list of uint8 planes."""
    return mspec.pyramid(frame, scale_of(mspec.scale_of() if scale is None else scale, exposures, f), levels)


def align(frames, exposures, ref, levels=mspec.DEFAULT_LEVELS, search=mspec.DEFAULT_SEARCH, zero_bias=DEFAULT_ZERO_BIAS, white_level=1.0):
    """MotionHdrMerge.align: (fields (F, Ty, Tx, 2) int16, costs (F, Ty, Tx, 2) uint32, the pyramids).  The rows of ref are not written
    by the device; here they are zero."""
    h, w = np.asarray(frames[0]).shape
    ny, nx = mspec.tiles(w, h)
    scale = mspec.scale_of(white_level)
    pyramids = [pyramid(x, exposures, f, scale, levels) for f, x in enumerate(frames)]
    fields, costs = np.zeros((len(frames), ny, nx, 2), np.int16), np.zeros((len(frames), ny, nx, 2), np.uint32)
    for f in range(len(frames)):
        if f != ref:
            fields[f], costs[f] = mspec.match(pyramids[ref], pyramids[f], w, h, search, zero_bias)
    return fields, costs, pyramids


def displaced(x, dy, dx):
    """x[q + (dy, dx)] for every site q, NaN where that lies outside the frame; and which sites lie inside."""
    h, w = x.shape
    i, j = np.indices((h, w))
    hi, hj = i + dy, j + dx
    inside = (hi >= 0) & (hi < h) & (hj >= 0) & (hj < w)
    out = np.full((h, w), np.nan, x.dtype)
    out[inside] = x[hi[inside], hj[inside]]
    return out, inside


def merge(frames, exposures, fields, model, pattern, ref, out_dtype=None, **kw):
    """One call of tdk_hdralign_merge: (out, mask).  The window of an output site evaluates every site it holds with the OUTPUT tile's
    displacements, so the bracket is merged once per distinct tuple of displacements and every tile takes its own."""
    frames = [np.asarray(x) for x in frames]
    nf, (h, w) = len(frames), frames[0].shape
    assert 0 <= ref < nf and np.asarray(fields).shape == (nf, *mspec.tiles(w, h), 2)
    out_dtype = frames[0].dtype if out_dtype is None else out_dtype
    masked = np.asarray(fields).astype(np.int64) & ~1
    masked[ref] = 0
    k, lo, _ = hspec.ratios(exposures, ref)
    out_all, mask_all = np.zeros((h, w), out_dtype), np.zeros((h, w), np.uint8)
    cache = {}
    ny, nx = mspec.tiles(w, h)
    for ty in range(ny):
        for tx in range(nx):
            D = tuple((int(masked[f, ty, tx, 0]), int(masked[f, ty, tx, 1])) for f in range(nf))
            if D not in cache:
                moved = [displaced(frames[f], *D[f]) for f in range(nf)]
                out, mask = hspec.merge([m[0] for m in moved], exposures, model, pattern, ref=ref, out_dtype=out_dtype, **kw)
                # rule 5: a site blown in every frame takes g = lo when its displaced sample lies inside the frame, else g = ref, which is
                # not displaced.  Exact behind the merge: a blown site takes part in no window and has no frame with weight.
                fix = ((mask & 8) != 0) & ~moved[lo][1]
                with np.errstate(all='ignore'):
                    R = (frames[ref].astype(F) / k[ref]).astype(out_dtype)
                out, mask = np.where(fix, R, out), np.where(fix, ref | 8, mask).astype(np.uint8)
                cache[D] = (out, mask)
            sl = (slice(TILE_H * ty, TILE_H * (ty + 1)), slice(TILE_W * tx, TILE_W * (tx + 1)))
            out_all[sl], mask_all[sl] = cache[D][0][sl], cache[D][1][sl]
    return out_all, mask_all


def process(frames, exposures, model, pattern, ref=None, levels=mspec.DEFAULT_LEVELS, search=mspec.DEFAULT_SEARCH, zero_bias=DEFAULT_ZERO_BIAS,
            white_level=1.0, **kw):
    """MotionHdrMerge.process with fields=None: (out, mask, fields, costs)."""
    ref = longest(exposures) if ref is None else ref
    fields, costs, _ = align(frames, exposures, ref, levels, search, zero_bias, white_level)
    out, mask = merge(frames, exposures, fields, model, pattern, ref, **kw)
    return out, mask, fields, costs
