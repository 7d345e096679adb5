"""GPU parity at BASELINE.json's full sizes (12 MP and 50 MP), through properties that do not
need a full-size oracle run:
  * crop consistency -- every op here has a bounded footprint, so the result on an interior
    window of the big frame must equal the oracle run on that window plus a margin (offsets
    chosen so CFA phase / tile grid / bilateral cells line up);
  * identities (native CFA sample preserved, sigma = 0, detail = 0, codec round trip)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W12, H12 = 4096, 3072
W50, H50 = 8192, 6144


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def frame12(dev):
    from torch_darktable.synthetic import synthetic_bayer

    return synthetic_bayer(H12, W12, seed=1234, device=dev)


def npy(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.float16 else t.detach().cpu().numpy()


def window(t, y0, x0, size, margin):
    """numpy copy of t[y0-margin : y0+size+margin, x0-margin : ...]"""
    return npy(t[y0 - margin:y0 + size + margin, x0 - margin:x0 + size + margin]).copy()


WINDOWS = [(1024, 2048), (2000, 304), (64, 3504)]  # (y0, x0): multiples of 8 (CFA phase, Wiener tile grid, bilateral cells)


def edge_windows(w, h, n=256):
    """(y0, y1, x0, x1): a window on the bottom edge, one on the right edge and the bottom-right corner.  They start on the last
    multiple of 8 that leaves at least n pixels and run to the frame's edge."""
    yb, xr = 8 * ((h - n) // 8), 8 * ((w - n) // 8)
    return [(yb, h, 1024, 1024 + n), (1024, 1024 + n, xr, w), (yb, h, xr, w)]


def edge_crop(t, win, margin):
    """numpy copy of the window plus `margin` on its inner sides (none past the frame's edge) and the window's offset in it."""
    y0, y1, x0, x1 = win
    h, w = t.shape[:2]
    cy0, cx0 = max(y0 - margin, 0), max(x0 - margin, 0)
    return npy(t[cy0:min(y1 + margin, h), cx0:min(x1 + margin, w)]).copy(), (slice(y0 - cy0, y1 - cy0), slice(x0 - cx0, x1 - cx0))


def test_rcd_12mp_crop_consistency_and_native(td, oracle, dev, frame12):
    out = td.RCD(dev, (W12, H12), td.BayerPattern.RGGB).process(frame12)
    assert out.shape == (H12, W12, 3)
    m, n = 16, 256
    for y0, x0 in WINDOWS:
        ref = oracle.rcd(window(frame12, y0, x0, n, m), oracle.RGGB)[m:-m, m:-m]
        got = npy(out[y0:y0 + n, x0:x0 + n])
        assert np.array_equal(got, ref), f'window {(y0, x0)}: max |d| {np.abs(got - ref).max()}'
    # native CFA sample survives everywhere (RGGB: R at even/even, B at odd/odd)
    assert torch.equal(out[0::2, 0::2, 0], frame12[0::2, 0::2, 0].clamp_min(0))
    assert torch.equal(out[1::2, 1::2, 2], frame12[1::2, 1::2, 0].clamp_min(0))
    assert torch.equal(out[0::2, 1::2, 1], frame12[0::2, 1::2, 0].clamp_min(0))
    assert torch.isfinite(out).all()


def test_rcd_12mp_fp16_fast_arithmetic(td, oracle, dev, frame12):
    """BASELINE config 3's demosaic: float16 storage, the approximate arithmetic flavour of the column strips (default for
    float16 results; csrc/tdk_rcd_stream.h) on the whole 12 MP frame.  Windows against the fp32 oracle rounded to binary16: at
    most one binary16 ulp except on <= 1e-5 of the pixels (selection flips); the register-blocked strips (what FrameStreams
    runs) give the same bits on every pixel of the frame; native samples pass through."""
    from torch_darktable import torch_darktable_extension as ext

    b16 = frame12.half()
    ws = td.RCD(dev, (W12, H12), td.BayerPattern.RGGB)
    out = ws.process(b16)
    with ext.concurrent_frames():
        quad = ws.process(b16)
    assert out.dtype == torch.float16 and torch.equal(out, quad)
    m, n = 16, 256
    beyond = touched = 0
    for y0, x0 in WINDOWS + [(m, m), (H12 - n - m, W12 - n - m)]:  # (the two corner windows: the crop's own border ring coincides with the frame's)
        ref = oracle.rcd(window(b16, y0, x0, n, m)[:, :, :1], oracle.RGGB)[m:-m, m:-m]
        got = npy(out[y0:y0 + n, x0:x0 + n])
        r16 = ref.astype(np.float16).astype(np.float32)
        d = np.abs(got - r16)
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(np.abs(got), np.abs(r16)), 2.0 ** -14))) - 10)
        beyond += int((d > ulp).any(-1).sum())
        touched += int((d > 0).sum())
    npx = 5 * n * n
    assert beyond <= 1e-5 * npx + 1 and touched <= 1e-3 * 3 * npx, (beyond, touched, npx)
    assert torch.equal(out[0::2, 0::2, 0], b16[0::2, 0::2, 0].clamp_min(0))
    assert torch.equal(out[1::2, 1::2, 2], b16[1::2, 1::2, 0].clamp_min(0))
    assert torch.isfinite(out).all()


def test_rcd_12mp_right_and_bottom_edges(td, oracle, dev, frame12):
    """The stale p/q slots of the reference's shared scratch planes influence the last columns /
    rows; check those against a full-width / full-height strip of the oracle is too costly, so
    use a smaller frame with the same width class instead (4096 wide, 96 tall)."""
    strip = frame12[:96].contiguous()
    got = npy(td.RCD(dev, (W12, 96), td.BayerPattern.RGGB).process(strip))
    assert np.array_equal(got, oracle.rcd(npy(strip), oracle.RGGB))


@pytest.mark.parametrize('shape', [(W12, H12), (W50, H50), (4096 + 2, 3072 - 31)])
def test_rcd_strips_equal_tiles_on_whole_frames(td, dev, shape):
    """The column strips (csrc/tdk_rcd_stream.h) and the 64 x 64 tile kernel must agree on EVERY pixel of a full-size frame --
    all strip and segment seams, the moved-back last strip / segment, the border rules on all four sides and the ring -- for
    fp32 and fp16 storage and a second CFA phase.  (The windows above tie the result to the oracle.)"""
    from torch_darktable import torch_darktable_extension as ext
    from torch_darktable.synthetic import synthetic_bayer

    w, h = shape
    bayer = synthetic_bayer(h, w, seed=77, device=dev)
    for pattern in (td.BayerPattern.RGGB, td.BayerPattern.GBRG):
        ws = td.RCD(dev, (w, h), pattern)
        for x in (bayer, bayer.half()):
            with ext.verification_paths(rcd_exact=True):  # (float16 results: the exact flavour rounded once, as the tile kernel's)
                strips = ws.process(x)
                with ext.concurrent_frames():  # the register-blocked strips (TDK_RCD_CONCURRENT)
                    quad = ws.process(x)
            with ext.verification_paths(rcd_tiles=True):
                tiles = ws.process(x)
            assert torch.equal(strips, tiles), f'{shape} {pattern} {x.dtype}: {(strips != tiles).sum().item()} values differ'
            assert torch.equal(quad, tiles), f'{shape} {pattern} {x.dtype}, register-blocked strips: {(quad != tiles).sum().item()} values differ'
            del strips, tiles, quad


def test_ppg_bilinear_12mp_crop_consistency(td, oracle, dev, frame12):
    ppg = td.PPG(dev, (W12, H12), td.BayerPattern.RGGB).process(frame12)
    bil = td.bilinear5x5_demosaic(frame12, td.BayerPattern.RGGB)
    m, n = 8, 256
    for y0, x0 in WINDOWS:
        w = window(frame12, y0, x0, n, m)
        assert np.array_equal(npy(ppg[y0:y0 + n, x0:x0 + n]), oracle.ppg(w, oracle.RGGB)[m:-m, m:-m])
        assert np.array_equal(npy(bil[y0:y0 + n, x0:x0 + n]), oracle.bilinear5x5(w, oracle.RGGB)[m:-m, m:-m])


def test_codec_12mp_roundtrip(td, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randint(0, 4096, (W12 * H12,), generator=g, device=dev, dtype=torch.int32).to(torch.uint16)
    packed = td.encode12_u16(x)
    assert packed.numel() == W12 * H12 * 3 // 2
    assert torch.equal(td.decode12_u16(packed).to(torch.int32), x.to(torch.int32))
    f = td.decode12_float(packed)
    assert torch.equal(td.decode12_u16(td.encode12_float(f)).to(torch.int32), x.to(torch.int32))
    assert torch.equal(td.decode12_half(packed), f.half())


def test_wiener_12mp(td, oracle, dev, frame12):
    rgb = td.RCD(dev, (W12, H12), td.BayerPattern.RGGB).process(frame12)
    ll = td.compute_log_luminance(rgb, 1e-4)
    ws = td.Wiener(dev, (W12, H12), overlap_factor=4, tile_size=32)
    ident = ws.process(ll.unsqueeze(2), 0.0)
    assert (ident.squeeze(2) - ll).abs().max().item() < 2e-5  # log-luminance spans [-9.2, 0]
    den = ws.process(ll.unsqueeze(2), 0.075).squeeze(2)
    m, n = 32, 256  # tile grid has period 8; a window is reproduced by any crop with a 32-px margin
    for y0, x0 in WINDOWS:
        ref = oracle.wiener(window(ll, y0, x0, n, m)[:, :, None], 0.075, 32, 4)[m:-m, m:-m, 0]
        got = npy(den[y0:y0 + n, x0:x0 + n])
        assert np.abs(got - ref).max() < 5e-5, f'window {(y0, x0)}: {np.abs(got - ref).max()}'


@pytest.mark.parametrize('shape', [(W12, H12), (4096 + 2, 3072 - 31)])
def test_wiener_12mp_right_and_bottom_edges(td, oracle, dev, shape):
    """The y-streaming kernel's last, partial segment of each strip (its length comes from pick_segment_rows, csrc/wiener.hip, and
    only big frames have one) and the frame's last tile row / column.  4098 x 3041: a partial last strip and the scalar load path
    (W % 4 != 0)."""
    from torch_darktable.synthetic import synthetic_bayer

    w, h = shape
    bayer = synthetic_bayer(h, w, seed=1234, device=dev)
    ll = td.compute_log_luminance(td.RCD(dev, (w, h), td.BayerPattern.RGGB).process(bayer), 1e-4)
    den = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32).process(ll.unsqueeze(2), 0.075).squeeze(2)
    for win in edge_windows(w, h):
        crop, (ys, xs) = edge_crop(ll, win, 32)
        ref = oracle.wiener(crop[:, :, None], 0.075, 32, 4)[ys, xs, 0]
        got = npy(den[win[0]:win[1], win[2]:win[3]])
        assert np.abs(got - ref).max() < 5e-5, f'{shape} window {win}: {np.abs(got - ref).max()}'


def test_bilateral_12mp(td, oracle, dev, frame12):
    rgb = td.RCD(dev, (W12, H12), td.BayerPattern.RGGB).process(frame12)
    lum = td.compute_luminance(rgb)
    ws = td.Bilateral(dev, (W12, H12), sigma_s=2.0, sigma_r=0.2)
    assert ws._bilateral.grid_size() == (2049, 1537, 6)
    assert torch.equal(ws.process(lum, 0.0), lum.clamp_min(0))
    out = ws.process(lum, 0.4)
    m, n = 16, 256  # cell = 2 px; splat 1 cell + blur 2 cells + slice 1 cell = 8 px < margin
    for y0, x0 in WINDOWS:
        ref = oracle.bilateral(window(lum, y0, x0, n, m), 2.0, 0.2, 0.4)[m:-m, m:-m]
        got = npy(out[y0:y0 + n, x0:x0 + n])
        assert np.array_equal(got, ref), f'window {(y0, x0)}: {np.abs(got - ref).max()}'
    win = edge_windows(W12, H12)[-1]  # the bottom-right corner: the grid's last cells on both axes
    crop, (ys, xs) = edge_crop(lum, win, m)
    got = npy(out[win[0]:win[1], win[2]:win[3]])
    ref = oracle.bilateral(crop, 2.0, 0.2, 0.4)[ys, xs]
    assert np.array_equal(got, ref), f'window {win}: {np.abs(got - ref).max()}'


def test_full_pipeline_12mp_fp16_vs_fp32_oracle(td, oracle, dev, frame12):
    """BASELINE config 3 (one frame of the batch): fp16 storage / fp32 arithmetic against the fp32 oracle chain on
    interior windows.  North-star tolerance for fp16 storage: 2e-3 RELATIVE.  The chain rounds to binary16 three times
    (RCD, Wiener and bilateral outputs; half an ulp = 2^-12 of the value each), and the two lightness replacements move
    every channel of a pixel together, so the error of a channel scales with the PIXEL (its largest channel), not with
    that channel alone: a dark channel of a bright pixel legitimately carries the bright channels' rounding.  Checked as
    |d| <= 2e-3 * max(R, G, B) per pixel; measured 1.4e-3 (profiles/r02/fp16_chain_error.json; the fp32-storage
    chain sits at 2e-6).  The uint8 output: +-2 LSB."""
    b16 = frame12.half()
    rgb = td.RCD(dev, (W12, H12), td.BayerPattern.RGGB).process(b16)
    den = td.Wiener(dev, (W12, H12)).process_log_luminance(rgb, 0.075)
    loc = td.Bilateral(dev, (W12, H12), sigma_s=2.0, sigma_r=0.2).process_rgb(den, 0.4)
    metrics = td.compute_image_metrics([loc], stride=8)
    u8 = td.reinhard_tonemap(loc, metrics, td.TonemapParameters(0.75, 2.0, 1.0, 0.0))
    assert u8.dtype == torch.uint8 and u8.shape == (H12, W12, 3)
    m, n = 64, 192
    y0, x0 = 1024, 2048
    bw = window(b16[:, :, 0], y0, x0, n, m).astype(np.float32)
    r = oracle.rcd(bw, oracle.RGGB)
    ll = oracle.compute_luminance(r, True, 1e-4)
    r = oracle.modify_luminance(r, oracle.wiener(ll[:, :, None], 0.075, 32, 4)[:, :, 0], True)
    r = oracle.modify_luminance(r, oracle.bilateral(oracle.compute_luminance(r), 2.0, 0.2, 0.4))
    ref_u8 = oracle.tonemap('reinhard', r, npy(metrics), 0.75, 2.0, 1.0, 0.0)[m:-m, m:-m]
    got_rgb = npy(loc[y0:y0 + n, x0:x0 + n])
    ref_rgb = r[m:-m, m:-m]
    rel = np.abs(got_rgb - ref_rgb) / np.maximum(ref_rgb.max(-1, keepdims=True), 1e-3)
    assert rel.max() < 2e-3, rel.max()
    # the stricter per-VALUE form of the same tolerance (each channel against itself, floor 0.05: below it the absolute
    # error of the pixel's brighter channels dominates): measured 1.5e-3 (profiles/r04/fp16_chain_error.json)
    rel_ch = np.abs(got_rgb - ref_rgb) / np.maximum(np.abs(ref_rgb), 0.05)
    assert rel_ch.max() < 2e-3, rel_ch.max()
    d = np.abs(npy(u8[y0:y0 + n, x0:x0 + n]).astype(np.int32) - ref_u8.astype(np.int32))
    assert d.max() <= 2 and (d > 1).mean() <= 1e-5, (d.max(), (d > 1).mean())  # measured: 8e-8 of the values above 1 LSB


def test_config5_50mp_ppg_wiener_fp16(td, oracle, dev):
    """BASELINE config 5: 8192 x 6144 RGGB, PPG demosaic + Wiener C=3 (K=32, ov=4, sigma=0.05;
    the reference has no wavelet denoiser), fp16 storage."""
    from torch_darktable.synthetic import synthetic_bayer

    bayer = synthetic_bayer(H50, W50, seed=77, device=dev).half()
    rgb = td.PPG(dev, (W50, H50), td.BayerPattern.RGGB).process(bayer)
    assert rgb.shape == (H50, W50, 3) and rgb.dtype == torch.float16
    assert torch.equal(rgb[0::2, 0::2, 0], bayer[0::2, 0::2, 0]) and torch.equal(rgb[1::2, 1::2, 2], bayer[1::2, 1::2, 0])
    m, n, y0, x0 = 8, 256, 3000, 6000
    ref = oracle.ppg(window(bayer[:, :, 0], y0, x0, n, m).astype(np.float32), oracle.RGGB)[m:-m, m:-m]
    assert np.array_equal(npy(rgb[y0:y0 + n, x0:x0 + n]), ref.astype(np.float16).astype(np.float32))
    ws = td.Wiener(dev, (W50, H50), overlap_factor=4, tile_size=32)
    den = ws.process(rgb, 0.05)
    assert den.shape == rgb.shape and torch.isfinite(den).all()
    m = 32
    refw = oracle.wiener(window(rgb, y0, x0, n, m), 0.05, 32, 4)[m:-m, m:-m]
    assert np.abs(npy(den[y0:y0 + n, x0:x0 + n]) - refw).max() < 2e-3  # fp16 output rounding
    win = edge_windows(W50, H50)[-1]  # the bottom-right corner: last strip, last segment, last tile row and column
    crop, (ys, xs) = edge_crop(rgb, win, m)
    refw = oracle.wiener(crop, 0.05, 32, 4)[ys, xs]
    assert np.abs(npy(den[win[0]:win[1], win[2]:win[3]]) - refw).max() < 2e-3
    ident = ws.process(rgb, 0.0)
    assert (ident.float() - rgb.float()).abs().max().item() < 2e-3
