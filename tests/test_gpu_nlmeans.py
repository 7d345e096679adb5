"""GPU: non-local means (torch_darktable.NLMeans, include/tdk_hip_denoise.h) against a NumPy restatement of its specification.

The operator has no reference implementation; `nlm_ref` below is the yardstick.  It evaluates the formulas as direct sums in the
order they are written, in float64 (`ref64`) or float32 (`ref32`):

    D(p, d) = 1/n sum_t sum_c cw[c] (x_c(clamp(p+t)) - x_c(clamp(p+d+t)))^2          n = (2P+1)^2
    w(p, d) = exp(-D / h^2) if p+d lies inside the image else 0
    y_c(p)  = sum_d w(p,d) x_c(p+d) / sum_d w(p,d)

Tolerance: for each case floor = max|ref32 - ref64| on that very input, and the GPU may be 4 x floor + 2^-23 away from ref64 --
the margin for a different summation order and the hardware exponential.  float16 storage: ref64 on the binary16-rounded input,
rounded once to binary16, within one binary16 ulp.  Every parity check prints its figures (pytest -s) before it asserts."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def nlm_ref(x, S, P, h, cw=None, dtype=np.float64, candidates='skip', patches='edge'):
    """The specification.  candidates='clamp' / patches='zero' are the two border rules it does NOT have (test_border_rules)."""
    x = x.astype(dtype)
    H, W, C = x.shape
    R = S + P
    cw = np.ones(C, dtype) if cw is None else np.asarray(cw, dtype)
    pad = np.pad(x, ((R, R), (R, R), (0, 0)), mode='edge' if patches == 'edge' else 'constant')   # patch samples
    val = np.pad(x, ((S, S), (S, S), (0, 0)), mode='edge')                                        # candidate values
    n, h2 = dtype((2 * P + 1) ** 2), dtype(h) * dtype(h)
    yy, xx = np.mgrid[0:H, 0:W]
    num, den = np.zeros((H, W, C), dtype), np.zeros((H, W), dtype)
    own = pad[S:S + H + 2 * P, S:S + W + 2 * P]
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            d = own - pad[S + dy:S + dy + H + 2 * P, S + dx:S + dx + W + 2 * P]
            e = (cw * (d * d)).sum(-1, dtype=dtype)
            D = np.zeros((H, W), dtype)
            for ty in range(2 * P + 1):
                for tx in range(2 * P + 1):
                    D = D + e[ty:ty + H, tx:tx + W]
            w = np.exp(-(D / n) / h2)
            if candidates == 'skip':
                w = np.where((yy + dy >= 0) & (yy + dy < H) & (xx + dx >= 0) & (xx + dx < W), w, dtype(0))
            num += w[..., None] * val[S + dy:S + dy + H, S + dx:S + dx + W]
            den += w
    out = num / den[..., None]
    assert out.dtype == dtype
    return out


def run(td, dev, x, S, P, h, cw=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = td.NLMeans(dev, (x.shape[1], x.shape[0]), S, P).process(t, h, cw)
    assert out.shape == t.shape and out.dtype == t.dtype
    return out.cpu().numpy()


WORST = {'err': 0.0, 'floor': 0.0}


def tolerance(x, S, P, h, cw, r64):
    floor = float(np.abs(nlm_ref(x, S, P, h, cw, np.float32).astype(np.float64) - r64).max())
    return floor, 4.0 * floor + 2.0 ** -23


def check_f32(td, dev, x, S, P, h, cw=None, what=''):
    r64 = nlm_ref(x, S, P, h, cw)
    floor, tol = tolerance(x, S, P, h, cw, r64)
    err = float(np.abs(run(td, dev, x, S, P, h, cw).astype(np.float64) - r64).max())
    WORST['err'], WORST['floor'] = max(WORST['err'], err), max(WORST['floor'], floor)
    print(f'nlmeans f32 {what}{x.shape} S={S} P={P} h={h} cw={cw}: gpu err {err:.3e} floor {floor:.3e} tol {tol:.3e} '
          f'(worst so far: err {WORST["err"]:.3e}, floor {WORST["floor"]:.3e})')
    assert err <= tol, (x.shape, S, P, h, cw, err, floor, tol)
    return r64, tol


def half_ulp(a, b):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -14))) - 10)


def check_f16(td, dev, x, S, P, h, cw=None):
    x16 = x.astype(np.float16)
    want = nlm_ref(x16, S, P, h, cw).astype(np.float16).astype(np.float32)
    got = run(td, dev, x16, S, P, h, cw)
    assert got.dtype == np.float16
    got = got.astype(np.float32)
    over = np.abs(got - want) > half_ulp(got, want)
    print(f'nlmeans f16 {x.shape} S={S} P={P} h={h} cw={cw}: {(got != want).mean():.2e} of the values differ, {int(over.sum())} by more than 1 ulp')
    assert not over.any(), (x.shape, S, P, h, cw, int(over.sum()))


def image(scene, h, w, c, seed=1234, noise=0.03):
    img = scene(h, w, seed, noise)
    return np.ascontiguousarray(img if c == 3 else img[:, :, 1:2])


HS = [0.03, 0.1, 0.5]
CWS = {1: [None, [0.5]], 3: [None, [1.0, 0.25, 0.0], [0.3, 2.0, 0.7]]}
RADII = [(S, P) for S in (1, 3, 7, 10) for P in (1, 2, 3, 4)]


# ------------------------------------------------------------------ 1. parity, float32
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('size', [(1, 1), (3, 5), (37, 53)])
def test_parity_f32_every_radius_on_images_smaller_than_the_window(td, dev, scene, size, c):
    """Every (S, P) of S in {1, 3, 7, 10} x P in 1..4 on frames smaller than the window in both axes, in one, or in neither; h and
    the channel weights (unequal, one of them zero) rotate through the cases."""
    x = image(scene, *size, c)
    for i, (S, P) in enumerate(RADII):
        check_f32(td, dev, x, S, P, HS[i % 3], CWS[c][(i // 3) % len(CWS[c])])
    if size == (1, 1):
        assert np.array_equal(run(td, dev, x, 7, 2, 0.1), x), 'a 1x1 image returns itself'


@pytest.mark.parametrize('size,c,S,P,h,cw', [
    ((250, 334), 3, 7, 2, 0.1, None), ((250, 334), 1, 10, 4, 0.03, None), ((250, 334), 3, 3, 1, 0.5, [1.0, 0.25, 0.0]),
    ((250, 334), 1, 1, 3, 0.1, [0.5]), ((257, 771), 3, 7, 2, 0.03, [0.3, 2.0, 0.7]), ((257, 771), 1, 3, 4, 0.5, None),
    ((257, 771), 3, 10, 1, 0.1, None), ((257, 771), 1, 7, 3, 0.03, None)])
def test_parity_f32_many_tiles(td, dev, scene, size, c, S, P, h, cw):
    check_f32(td, dev, image(scene, *size, c), S, P, h, cw)


# ------------------------------------------------------------------ 2. parity, float16 storage
@pytest.mark.parametrize('size,c,S,P,h,cw', [
    ((1, 1), 3, 7, 2, 0.1, None), ((3, 5), 1, 10, 4, 0.1, None), ((37, 53), 3, 7, 2, 0.1, [1.0, 0.25, 0.0]), ((37, 53), 1, 3, 1, 0.03, None),
    ((37, 53), 3, 10, 3, 0.5, None), ((250, 334), 3, 7, 2, 0.1, None), ((257, 771), 1, 5, 4, 0.03, [0.5]), ((257, 771), 3, 1, 1, 0.1, None)])
def test_parity_f16_storage(td, dev, scene, size, c, S, P, h, cw):
    check_f16(td, dev, image(scene, *size, c), S, P, h, cw)


# ------------------------------------------------------------------ 3. the two border rules
@pytest.mark.parametrize('c', [1, 3])
def test_border_rules_discriminate(td, dev, c):
    """A strong edge two pixels inside the frame's border, on all four sides.  Replicating the candidates instead of skipping
    them, or zero-padding the patch samples instead of replicating them, moves the result by far more than the tolerance (checked
    on the CPU first); the GPU follows the specified rules."""
    rng = np.random.default_rng(5)
    H, W, S, P, h = 24, 30, 3, 2, 0.25
    x = np.full((H, W, c), 0.25, np.float32)
    x[:2], x[-2:], x[:, :2], x[:, -2:] = 0.9, 0.8, 0.85, 0.95
    x = (x + rng.normal(0, 0.02, x.shape)).astype(np.float32)
    r64 = nlm_ref(x, S, P, h)
    floor, tol = tolerance(x, S, P, h, None, r64)
    for rule in ({'candidates': 'clamp'}, {'patches': 'zero'}):
        moved = float(np.abs(nlm_ref(x, S, P, h, **rule) - r64).max())
        print(f'nlmeans border rule {rule}: moves the result by {moved:.3e}, tolerance {tol:.3e}')
        assert moved > 100 * tol, (rule, moved, tol)
    err = float(np.abs(run(td, dev, x, S, P, h).astype(np.float64) - r64).max())
    print(f'nlmeans border rules: gpu err {err:.3e} floor {floor:.3e} tol {tol:.3e}')
    assert err <= tol, (err, tol)


# ------------------------------------------------------------------ 4. full size
def big_frame(dev, h, w, c, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(h, 1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, w, 1)
    ph = torch.arange(c, device=dev, dtype=torch.float32).view(1, 1, c)
    img = 0.5 + 0.3 * torch.sin(xx / 23.0 + ph) * torch.cos(yy / 17.0 - ph) + 0.15 * (((xx // 96) + (yy // 80)) % 2)
    img += torch.randn(img.shape, generator=g, device=dev) * 0.03
    return img.clamp_(0.0, 1.0).to(dtype).contiguous()


def windows(h, w, n=40):
    """(y0, y1, x0, x1): three interior windows (one across a tile seam of every tile width in use), one on each edge, one corner."""
    return [(1000, 1000 + n, 2040, 2040 + n), (h // 2 - 7, h // 2 - 7 + n, 301, 301 + n), (61, 61 + n, w - 600, w - 600 + n),
            (0, n, 1500, 1500 + n), (h - n, h, 777, 777 + n), (1300, 1300 + n, 0, n), (900, 900 + n, w - n, w), (h - n, h, w - n, w)]


def check_windows(td, dev, frame, S, P, h):
    H, W, C = frame.shape
    out = td.NLMeans(dev, (W, H), S, P).process(frame, h)
    assert out.shape == frame.shape and out.dtype == frame.dtype
    m = S + P   # the reference on the window grown by S + P (not past the frame) is exact on the window
    for y0, y1, x0, x1 in windows(H, W):
        cy0, cx0 = max(y0 - m, 0), max(x0 - m, 0)
        crop = frame[cy0:min(y1 + m, H), cx0:min(x1 + m, W)].cpu().numpy()
        inner = (slice(y0 - cy0, y1 - cy0), slice(x0 - cx0, x1 - cx0))
        got = out[y0:y1, x0:x1].cpu().numpy()
        if frame.dtype == torch.float16:
            want = nlm_ref(crop, S, P, h)[inner].astype(np.float16).astype(np.float32)
            got = got.astype(np.float32)
            over = np.abs(got - want) > half_ulp(got, want)
            print(f'nlmeans f16 {tuple(frame.shape)} window {(y0, x0)}: {int(over.sum())} values beyond 1 ulp')
            assert not over.any(), (y0, x0, int(over.sum()))
        else:
            r64 = nlm_ref(crop, S, P, h)
            floor = float(np.abs(nlm_ref(crop, S, P, h, None, np.float32).astype(np.float64) - r64)[inner].max())
            tol = 4.0 * floor + 2.0 ** -23
            err = float(np.abs(got.astype(np.float64) - r64[inner]).max())
            WORST['err'], WORST['floor'] = max(WORST['err'], err), max(WORST['floor'], floor)
            print(f'nlmeans f32 {tuple(frame.shape)} window {(y0, x0)}: gpu err {err:.3e} floor {floor:.3e} tol {tol:.3e}')
            assert err <= tol, (y0, x0, err, tol)


@pytest.mark.parametrize('h,w,c,dtype', [(3072, 4096, 3, torch.float32), (3072, 4096, 3, torch.float16), (3072, 4096, 1, torch.float32),
                                         (3041, 4098, 3, torch.float32), (6144, 8192, 1, torch.float32)])
def test_full_size_windows(td, dev, h, w, c, dtype):
    """12 MP (float32 and float16), 4098 x 3041 (a frame that is no multiple of the tile) and 50 MP, at (S, P) = (7, 2)."""
    check_windows(td, dev, big_frame(dev, h, w, c, dtype, seed=h + c), 7, 2, 0.1)


# ------------------------------------------------------------------ 5. views at any element offset, any width
@pytest.mark.parametrize('dtype,offset', [(torch.float32, 4), (torch.float32, 8), (torch.float16, 2), (torch.float16, 4), (torch.float16, 8)])
@pytest.mark.parametrize('size', [(37, 53), (35, 54), (37, 51), (64, 128)])   # npix % 4 = 1, 2, 3, 0
def test_offset_views_and_pixel_tails(td, dev, scene, dtype, offset, size):
    """A contiguous view that starts 2, 4 or 8 bytes past an aligned allocation gives the bits of the aligned call, at widths
    with every npix % 4; the kernel has one element-wise load / store path, and this holds it to that."""
    for c in (1, 3):
        x = torch.from_numpy(image(scene, *size, c)).to(dev).to(dtype)
        nlm = td.NLMeans(dev, (size[1], size[0]), 5, 2)
        aligned = nlm.process(x, 0.1)
        assert x.data_ptr() % 16 == 0
        skip = offset // x.element_size()
        pool = torch.zeros(x.numel() + 16, dtype=dtype, device=dev)
        view = pool[skip:skip + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.data_ptr() % 16 == offset and view.is_contiguous()
        assert torch.equal(nlm.process(view, 0.1), aligned), (dtype, offset, size, c)
        assert torch.count_nonzero(pool[:skip]) == 0 and torch.count_nonzero(pool[skip + x.numel():]) == 0
    if dtype == torch.float32 and offset == 4:
        check_f32(td, dev, image(scene, *size, 3), 5, 2, 0.1)


# ------------------------------------------------------------------ 6. determinism, streams, graphs
def test_two_calls_give_identical_bits(td, dev, scene):
    x = torch.from_numpy(image(scene, 250, 334, 3)).to(dev)
    nlm = td.NLMeans(dev, (334, 250))
    a, b = nlm.process(x, 0.1), nlm.process(x, 0.1)
    assert torch.equal(a, b)
    assert torch.equal(td.NLMeans(dev, (334, 250)).process(x.clone(), 0.1), a)


def test_three_frames_on_three_streams_equal_their_serial_results(td, dev, scene):
    frames = [torch.from_numpy(image(scene, 600, 800, 3, seed=s)).to(dev) for s in (1, 2, 3)]
    nlm = td.NLMeans(dev, (800, 600))
    serial = [nlm.process(f, 0.1) for f in frames]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in frames]
    for _ in range(2):
        outs = []
        for f, s in zip(frames, streams):
            with torch.cuda.stream(s):
                outs.append(nlm.process(f, 0.1))
        torch.cuda.synchronize()
        for o, want in zip(outs, serial):
            assert torch.equal(o, want)


def test_graph_capture_and_replay_on_changing_contents(td, dev, scene):
    """Captured on its first call (nothing to warm up: no allocation of its own, no copy, no synchronisation) and replayed on
    three different frames through the same input buffer."""
    frames = [torch.from_numpy(image(scene, 250, 334, 3, seed=s)).to(dev) for s in (11, 12, 13)]
    nlm = td.NLMeans(dev, (334, 250), 5, 3)
    cw = [1.0, 0.5, 0.25]
    static_in = torch.zeros_like(frames[0])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            static_out = nlm.process(static_in, 0.1, cw)
    torch.cuda.current_stream(dev).wait_stream(side)
    for f in frames:
        static_in.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, nlm.process(f, 0.1, cw))


# ------------------------------------------------------------------ 7. compositions and limits
def test_luminance_forms_are_the_hand_written_composition(td, dev, scene):
    rgb = torch.from_numpy(image(scene, 250, 334, 3)).to(dev)
    nlm = td.NLMeans(dev, (334, 250), 5, 2)
    lum = td.compute_luminance(rgb)
    want = td.modify_luminance(rgb, nlm.process(lum.unsqueeze(2), 0.05).squeeze(2))
    assert torch.equal(nlm.process_luminance(rgb, 0.05), want)
    log = td.compute_log_luminance(rgb, 1e-3)
    want = td.modify_log_luminance(rgb, nlm.process(log.unsqueeze(2), 0.2).squeeze(2), 1e-3)
    assert torch.equal(nlm.process_log_luminance(rgb, 0.2, eps=1e-3), want)
    log = td.compute_log_luminance(rgb, 1e-4)
    want = td.modify_log_luminance(rgb, nlm.process(log.unsqueeze(2), 0.2).squeeze(2), 1e-4)
    assert torch.equal(nlm.process_log_luminance(rgb, 0.2), want)
    assert not torch.equal(want, rgb)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_constant_image_returns_itself_exactly(td, dev, dtype):
    """w(p, 0) = 1 and every difference is zero: no rounding at all, for a value whose multiples are not exact in binary."""
    for c, size in ((1, (70, 130)), (3, (33, 61))):
        x = torch.full((*size, c), 0.3, dtype=dtype, device=dev)
        if c == 3:
            x[:, :, 1], x[:, :, 2] = 0.7, 1e-3
        assert torch.equal(td.NLMeans(dev, (size[1], size[0]), 10, 4).process(x, 0.05), x)


def test_large_h_is_the_mean_of_the_valid_search_window(td, dev, scene):
    x = image(scene, 37, 53, 3)
    S, P = 3, 2
    H, W, C = x.shape
    mean = np.zeros((H, W, C))
    for yy in range(H):
        for xx in range(W):
            mean[yy, xx] = x[max(yy - S, 0):yy + S + 1, max(xx - S, 0):xx + S + 1].astype(np.float64).mean((0, 1))
    for h in (1e3, 1e6):   # at 1e6 float32 cannot tell a weight from 1
        r64, tol = check_f32(td, dev, x, S, P, h, what='large h ')
        # values in [0, 1]: D <= C, every weight within C / h^2 of 1, the weighted mean within 2 C / h^2 of the plain one; with the
        # parity check above the GPU is then within tol + 2 C / h^2 of the mean
        assert np.abs(r64 - mean).max() <= 2.0 * C / h ** 2
