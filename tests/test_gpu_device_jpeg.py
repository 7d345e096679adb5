"""GPU: the device-resident JPEG encode (torch_darktable.device_jpeg, include/tdk_hip_ext.h).  The stream equals Jpeg.encode's and the
oracle's byte for byte, the device-built Huffman tables equal a restatement of T.81 K.2 / K.3, the call runs inside a captured HIP
graph (it never synchronises), a stream that does not fit reports -1 and writes nothing beyond the buffer, and several frames, objects,
streams and host threads keep out of each other's way."""

import io
import threading

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def sample_image(h, w, seed=0, noise=6.0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 100 * np.sin(xx / 17.0) * np.cos(yy / 23.0), 127 + 90 * np.sin((xx + yy) / 31.0), 127 + 80 * np.cos(xx / 11.0 - yy / 7.0)], -1)
    return np.clip(img + rng.normal(0, noise, img.shape), 0, 255).astype(np.uint8)


def arrange(img, fmt):
    """RGB (H, W, 3) -> the layout of input format fmt (0 BGR planar, 1 RGB planar, 2 BGRI, 3 RGBI)."""
    a = img if fmt & 1 else img[:, :, ::-1]
    return np.ascontiguousarray(a.transpose(2, 0, 1) if fmt < 2 else a)


def decode(stream):
    im = Image.open(io.BytesIO(bytes(stream)))
    im.load()
    return im


# ---------------------------------------------------------------- 1. bytes
@pytest.mark.parametrize('h,w', [(1, 1), (3, 2), (8, 8), (17, 9), (64, 96), (203, 331), (100, 2100), (520, 1030)])
@pytest.mark.parametrize('sub', [0, 1, 2])
@pytest.mark.parametrize('progressive', [False, True])
def test_stream_identical_to_jpeg_encode_and_oracle(td, oracle, dev, h, w, sub, progressive):
    img = sample_image(h, w, h * 7 + w)
    enc, host = td.DeviceJpeg(), td.Jpeg()
    for quality, fmt in ((94, 3), (35, 2), (100, 1), (75, 0)):
        x = torch.from_numpy(arrange(img, fmt)).to(dev)
        got = enc.encode(x, quality, fmt, sub, progressive).to_host().numpy()
        want = oracle.jpeg_encode(arrange(img, fmt), quality, fmt, sub, progressive)
        assert got.shape == want.shape and np.array_equal(got, want), (quality, fmt, got.shape, want.shape)
        assert np.array_equal(got, host.encode(x, quality, fmt, sub, progressive).numpy()), (quality, fmt)
    im = decode(got)
    assert im.size == (w, h) and im.mode == ('L' if sub == 2 else 'RGB')


def test_tonemapped_12mp_on_a_side_stream(td, oracle, dev):
    from torch_darktable.synthetic import synthetic_rgb

    h, w = 3072, 4096
    side = torch.cuda.Stream(device=dev)
    rgb = synthetic_rgb(h, w, 5, dev, 0.01)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):   # producer and encoder on the side stream, not synchronised in between
        u8 = td.aces_tonemap(rgb, td.TonemapParameters(1.0, 0.0, 0.8, 0.0))
        res = td.DeviceJpeg().encode(u8, 94, td.InputFormat.RGBI, td.Subsampling.CSS_422, False)
    data = res.to_host().numpy()   # from the default stream: waits for the side stream
    assert np.array_equal(data, oracle.jpeg_encode(u8.cpu().numpy(), 94, 3, 1, False))
    assert decode(data).size == (w, h)


def test_50mp_frame(td, oracle, dev):
    from torch_darktable.synthetic import synthetic_rgb

    h, w = 6144, 8192
    u8 = td.aces_tonemap(synthetic_rgb(h, w, 9, dev, 0.01), td.TonemapParameters(1.0, 0.0, 0.8, 0.0))
    data = td.DeviceJpeg().encode(u8, 90, td.InputFormat.RGBI, td.Subsampling.CSS_422, False).to_host().numpy()
    want = oracle.jpeg_encode(u8.cpu().numpy(), 90, 3, 1, False)
    assert data.shape == want.shape and np.array_equal(data, want)


# ---------------------------------------------------------------- 2. tables
def k2_table(counts):
    """T.81 K.2 (figures K.1 - K.4, ties towards the larger symbol) and K.3, HUFFVAL by (code size, symbol), canonical codes:
    (BITS[1..16], HUFFVAL, packed[256] = code << 8 | length)."""
    freq = [int(c) for c in counts] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        v = None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        v = None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 64
    for c in codesize:
        if c:
            bits[min(c, 63)] += 1
    for i in range(63, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for length in range(1, 64) for s in range(256) if codesize[s] == length]
    packed = [0] * 256
    code = k = 0
    for length in range(1, 17):
        for _ in range(bits[length]):
            packed[vals[k]] = (code << 8) | length
            code += 1
            k += 1
        code <<= 1
    return bits[1:17], vals, packed


def table_cases():
    rng = np.random.default_rng(2024)
    cases = {}
    one = np.zeros(256, np.uint32)
    one[37] = 5
    cases['single symbol'] = one
    one1 = np.zeros(256, np.uint32)
    one1[0] = 1
    cases['single symbol, count 1 (ties the reserved one)'] = one1
    two = np.zeros(256, np.uint32)
    two[[3, 200]] = [7, 7]
    cases['two symbols'] = two
    cases['all 256 equal'] = np.full(256, 1000, np.uint32)
    fib = np.zeros(256, np.uint32)
    a, b = 1, 1
    for s in range(45):   # lengths far beyond 16: K.3 has to fold them
        fib[(s * 37) % 256] = a
        a, b = b, a + b
    cases['fibonacci'] = fib
    cases['sum past 2^32'] = rng.integers(2**31, 2**32, 256, dtype=np.uint64).astype(np.uint32)
    for k in range(6):
        t = rng.integers(0, 4, 256).astype(np.uint32)   # few distinct counts: ties everywhere
        t[rng.random(256) < 0.3 * k / 5] = 0
        cases[f'ties {k}'] = t
    dc = np.zeros(256, np.uint32)
    dc[:12] = rng.integers(1, 100000, 12)
    cases['dc-like'] = dc
    return cases


def test_device_tables_equal_k2_k3_restatement(td, dev):
    from torch_darktable._native import lib
    from torch_darktable.torch_darktable_extension import _ptr, _stream, check

    cases = table_cases()
    counts = torch.from_numpy(np.stack(list(cases.values())).view(np.int32)).to(dev)   # uint32 bits in int32 storage
    n = counts.shape[0]
    bits_vals = torch.zeros((n, 272), dtype=torch.uint8, device=dev)
    packed = torch.zeros((n, 256), dtype=torch.int32, device=dev)
    check(lib.tdk_jpeg_huffman_tables(_ptr(counts), n, _ptr(bits_vals), _ptr(packed), _stream()))
    bv, pk = bits_vals.cpu().numpy(), packed.cpu().numpy().view(np.uint32)
    for k, (name, c) in enumerate(cases.items()):
        bits, vals, want_packed = k2_table(c)
        assert list(bv[k, :16]) == bits, name
        assert list(bv[k, 16:16 + len(vals)]) == vals and not bv[k, 16 + len(vals):].any(), name
        assert list(pk[k]) == want_packed, name


# ---------------------------------------------------------------- 3. no synchronisation: graph capture
@pytest.mark.parametrize('progressive', [False, True])
def test_encode_replays_in_a_hip_graph(td, dev, progressive):
    h, w = 203, 331
    enc = td.DeviceJpeg()
    x = torch.from_numpy(sample_image(h, w, 1)).to(dev)
    buf = torch.empty(td.DeviceJpeg.max_stream_bytes(w, h, 1, progressive), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):   # warm-up on the capture's stream: the workspace is cached per (geometry, stream)
        enc.encode(x, 90, 3, 1, progressive, out=buf)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = enc.encode(x, 90, 3, 1, progressive, out=buf)
    for seed in (2, 3, 2):
        x.copy_(torch.from_numpy(sample_image(h, w, seed, noise=4.0 * seed)).to(dev))
        graph.replay()
        want = td.Jpeg().encode(x, 90, 3, 1, progressive)
        assert torch.equal(res.to_host(), want), seed


def test_frame_streams_batch_ending_in_the_encoder_replays(td, dev):
    """Mosaic -> tone-mapped frame -> JPEG bytes on the device, three frames on three streams, captured as ONE graph by
    FrameStreams.capture and replayed on new mosaics: every frame's stream equals the eager chain's Jpeg.encode."""
    from torch_darktable.sharding import FrameStreams
    from torch_darktable.synthetic import synthetic_bayer

    h, w = 384, 512
    params = td.TonemapParameters(gamma=0.75, intensity=2.0, light_adapt=1.0, vibrance=0.0)

    def make_chain():
        rcd = td.RCD(dev, (w, h), td.BayerPattern.RGGB)
        enc = td.DeviceJpeg()
        return lambda bayer: enc.encode(td.aces_tonemap(rcd.process(bayer), params), 92, td.InputFormat.RGBI, td.Subsampling.CSS_422, False)

    eager_rcd = td.RCD(dev, (w, h), td.BayerPattern.RGGB)
    runner = FrameStreams(dev, make_chain, streams=3)
    static = [synthetic_bayer(h, w, seed=10 + i, device=dev) for i in range(3)]
    cap = runner.capture(static)
    for seeds in ((20, 21, 22), (30, 31, 32)):
        batch = [synthetic_bayer(h, w, seed=s, device=dev) for s in seeds]
        outs = cap.replay(batch)
        torch.cuda.synchronize()
        for i, (res, b) in enumerate(zip(outs, batch)):
            want = td.Jpeg().encode(td.aces_tonemap(eager_rcd.process(b), params), 92, 3, 1, False)
            assert torch.equal(res.to_host(), want), (seeds, i)


# ---------------------------------------------------------------- 4. overflow
def test_overflow_reports_minus_one_and_writes_nothing_beyond(td, oracle, dev):
    from torch_darktable.device_jpeg import retrieve

    rng = np.random.default_rng(5)
    img = (rng.integers(0, 2, (96, 128, 3)) * 255).astype(np.uint8)   # binary noise at quality 100: a large stream
    x = torch.from_numpy(img).to(dev)
    enc = td.DeviceJpeg()
    for progressive in (False, True):
        want = oracle.jpeg_encode(img, 100, 3, 0, progressive)
        for cap in (0, 100, 700, len(want) // 2, len(want) - 1):   # inside the header, the tables, the first scan's data, the EOI
            buf = torch.full((cap + 8192,), 0xA5, dtype=torch.uint8, device=dev)
            res = enc.encode(x, 100, 3, 0, progressive, out=buf[:cap])
            assert int(res.length.item()) == -1, (progressive, cap)
            assert bool((buf[cap:] == 0xA5).all()), (progressive, cap)
            with pytest.raises(td.JpegException):
                res.to_host()
            with pytest.raises(td.JpegException):
                retrieve([res])
        ok = enc.encode(x, 100, 3, 0, progressive)   # the same object afterwards, with room: the right bytes
        assert np.array_equal(ok.to_host().numpy(), want)
    want = oracle.jpeg_encode(img, 100, 3, 0, False)
    exact = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device=dev)
    res = enc.encode(x, 100, 3, 0, False, out=exact[:len(want)])   # a buffer of exactly the stream's length is enough
    assert np.array_equal(res.to_host().numpy(), want) and bool((exact[len(want):] == 0xA5).all())


# ---------------------------------------------------------------- 5. batches and concurrency
def test_four_frames_then_one_retrieve(td, oracle, dev):
    from torch_darktable.device_jpeg import retrieve

    imgs = [sample_image(120 + 8 * k, 200 + 24 * k, 60 + k) for k in range(4)]
    enc = td.DeviceJpeg()
    results = [enc.encode(torch.from_numpy(im).to(dev), 88, 3, k % 3, k == 3) for k, im in enumerate(imgs)]   # no synchronisation in between
    got = retrieve(results)
    assert len(got) == 4
    for k, (g, im) in enumerate(zip(got, imgs)):
        assert g.device.type == 'cpu' and np.array_equal(g.numpy(), oracle.jpeg_encode(im, 88, 3, k % 3, k == 3)), k
    same = [enc.encode(torch.from_numpy(imgs[0]).to(dev), 88, 3, 0, False) for _ in range(3)]   # one geometry, one workspace, three results
    assert all(np.array_equal(g.numpy(), got[0].numpy()) for g in retrieve(same))


def test_two_objects_on_two_threads_and_streams(td, oracle, dev):
    imgs = [sample_image(200 + 8 * k, 300 + 16 * k, 40 + k) for k in range(2)]
    want = [oracle.jpeg_encode(im, 90, 3, k + 1, k == 1) for k, im in enumerate(imgs)]
    errors = []

    def worker(k):
        try:
            stream = torch.cuda.Stream(device=dev)
            coder = td.DeviceJpeg()
            x = torch.from_numpy(imgs[k]).to(dev)
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(stream):
                results = [coder.encode(x, 90, td.InputFormat.RGBI, k + 1, k == 1) for _ in range(6)]
                for r in results:
                    got = r.to_host().numpy()
                    if not np.array_equal(got, want[k]):
                        errors.append((k, got.shape, want[k].shape))
                        return
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---------------------------------------------------------------- 6. API
def test_api_errors_raise_before_any_launch(td, dev):
    enc = td.DeviceJpeg()
    img = torch.from_numpy(sample_image(32, 48)).to(dev)
    res = enc.encode(img)   # the defaults of Jpeg.encode
    assert res.data.dtype == torch.uint8 and res.data.dim() == 1 and res.data.device == img.device
    assert res.data.numel() == td.DeviceJpeg.max_stream_bytes(48, 32, td.Subsampling.CSS_422, False)
    assert res.length.dim() == 0 and res.length.dtype == torch.int64 and res.length.device == img.device
    assert torch.equal(res.to_host(), td.Jpeg().encode(img))
    for bad, match in ((img.cpu(), 'CUDA'), (img.float(), 'uint8'), (img.permute(1, 0, 2), 'contiguous'), (img[:, :, :2].contiguous(), 'interleaved'),
                       (img, 'planar')):
        with pytest.raises(RuntimeError, match=match):
            enc.encode(bad, 90, td.InputFormat.RGB if match == 'planar' else td.InputFormat.RGBI, td.Subsampling.CSS_444, False)
    with pytest.raises(RuntimeError):
        enc.encode(img, 90, 7, td.Subsampling.CSS_444, False)
    for out, match in ((torch.empty(1 << 16, dtype=torch.float32, device=dev), 'uint8'), (torch.empty(1 << 16, dtype=torch.uint8), 'device'),
                       (torch.empty((2, 1 << 15), dtype=torch.uint8, device=dev), '1-D')):
        with pytest.raises(RuntimeError, match=match):
            enc.encode(img, 90, 3, 1, False, out=out)
    for q in (0, 101):
        with pytest.raises(td.JpegException, match='quality'):
            enc.encode(img, q)
