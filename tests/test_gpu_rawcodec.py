"""GPU: the lossless raw codec (torch_darktable.RawCodec, include/tdk_hip_rawcodec.h) against the NumPy restatement of the format,
tests/rawcodec_spec.py (held to literal loops in tests/test_rawcodec_spec.py).

Every byte of the stream up to its length, the length, every decoded sample, every bit of the float outputs and every packed byte must
be the restatement's: there is no tolerance in this file.  Shapes are sized by the span (64 sites), the segment (512 sites, one wave)
and the rounds of the scan (4096 segments): one site, one pair, two sites around a span and a segment boundary, odd widths (a row that
starts at an odd element, a lane with one site), more segments than one round of the scan takes.  The packed forms need an even number of
sites and are checked on every shape of the list that has one, and on odd widths whose pairs reach into the next row and the next segment.

The streams that raise a status bit are built so that an altered offset or width, even if followed blindly, stays inside the tensor of
max_stream_bytes they live in: the stream is a view of the head of that tensor."""
import struct

import numpy as np
import pytest
import torch

import rawcodec_spec as spec

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS = (1, 2, 62, 64, 66, 127, 130, 510, 512, 514, 1030), (1, 2, 5)
SHAPES = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(256, 1024)]
TALL = (2, 4100)   # 4100 segments: a second round of the scan; two content classes, for the time the restatement takes
GUARD = 0xA5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def upload(a, dev, offset=0):
    """A contiguous device tensor with the contents of `a` that starts `offset` elements behind an allocation's first byte."""
    flat = np.array(a).reshape(-1)   # (a copy: the shared references are read-only)
    buf = torch.empty(flat.size + offset, dtype=torch.from_numpy(flat[:1]).dtype, device=dev)
    buf[offset:].copy_(torch.from_numpy(flat))
    return buf[offset:].view(a.shape)


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int16)


_STREAMS = {}


def reference(kind, w, h, bits_=12, twelve=False):
    """(frame, the spec's stream), computed once per case and never written to."""
    key = (kind, w, h, bits_, twelve)
    if key not in _STREAMS:
        x = spec.frame(kind, w, h)
        x = spec.as_12bit(x) if twelve else x
        stream = spec.encode(x, bits_)
        x.setflags(write=False), stream.setflags(write=False)
        _STREAMS[key] = (x, stream)
    return _STREAMS[key]


def encoded(res):
    """(the stream's bytes up to its length, the length) of a RawCodecResult."""
    n = int(res.length.item())
    return host(res.data[:max(n, 0)]), n


@pytest.mark.parametrize('w,h', SHAPES + [TALL], ids=lambda v: str(v))
def test_stream_is_the_spec_and_comes_back(td, dev, w, h):
    codec = td.RawCodec(dev, (w, h), bits=16)
    assert codec.table_bytes() == spec.table_bytes(w, h) and codec.max_stream_bytes() == spec.max_stream_bytes(w, h)
    for kind in (('uniform', 'ramp') if (w, h) == TALL else spec.CLASSES):
        x, want = reference(kind, w, h, 16)
        res = codec.encode(upload(x, dev))
        got, n = encoded(res)
        assert n == want.size, (kind, n, want.size)
        assert np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:8])
        back, status = codec.decode(res, return_status=True)
        assert back.dtype == torch.uint16 and tuple(back.shape) == (h, w) and int(status.item()) == 0, kind
        assert np.array_equal(host(back), x), kind
        # a stream the spec produced, its whole length the tensor's
        back, status = codec.decode(upload(want, dev), return_status=True)
        assert int(status.item()) == 0 and np.array_equal(host(back), x), kind
        if kind == 'constant':
            assert n == codec.table_bytes()


@pytest.mark.parametrize('w,h', SHAPES, ids=lambda v: str(v))
def test_float_outputs_have_the_bits_of_decode12(td, dev, w, h):
    codec = td.RawCodec(dev, (w, h), bits=16)
    for kind in spec.CLASSES:   # every uint16 value: the restatement's one float32 product, rounded once more for binary16
        x, stream = reference(kind, w, h, 16)
        data = upload(stream, dev)
        f32, f16 = codec.decode(data, output=torch.float32), codec.decode(data, output=torch.float16)
        assert f32.dtype == torch.float32 and f16.dtype == torch.float16 and tuple(f32.shape) == tuple(f16.shape) == (h, w)
        assert np.array_equal(bits(host(f32)), bits(spec.to_float32(x))), kind
        assert np.array_equal(bits(host(f16)), bits(spec.to_float16(x))), kind
    if (w * h) % 2 == 0:   # ... and the kernels themselves on the packed bytes of the same samples (a packed buffer knows no rows: any even count)
        for kind in spec.CLASSES:
            x, stream = reference(kind, w, h, 12, twelve=True)
            data = upload(stream, dev)
            for ids in (False, True):
                packed = upload(spec.pack12(x, ids), dev)
                assert torch.equal(codec.decode(data, output=torch.float32).reshape(-1), td.decode12_float(packed, ids_format=ids)), (kind, ids)
                assert torch.equal(codec.decode(data, output=torch.float16).reshape(-1), td.decode12_half(packed, ids_format=ids)), (kind, ids)


# an odd width: a pair reaches into the next row (every even row) and, from 513 sites on, into the next segment of an odd row
ODD_PACKED = [(3, 2), (63, 4), (513, 2), (1025, 4), (1151, 6)]


@pytest.mark.parametrize('w,h', [s for s in SHAPES if (s[0] * s[1]) % 2 == 0] + ODD_PACKED, ids=lambda v: str(v))
def test_packed_frames_in_both_nibble_orders(td, dev, w, h):
    codec = td.RawCodec(dev, (w, h))
    for kind in spec.CLASSES:   # (the low 12 bits of every class)
        x, want = reference(kind, w, h, 12, twelve=True)
        for fmt, ids in ((td.PackedFormat.Packed12, False), (td.PackedFormat.Packed12_IDS, True)):
            payload = spec.pack12(x, ids)
            assert np.array_equal(spec.unpack12(payload, ids), x.reshape(-1))
            src = upload(payload, dev)
            assert np.array_equal(host(td.decode12_u16(src, ids_format=ids)), x.reshape(-1))   # the samples are those of tdk_decode12_u16
            res = codec.encode(src, packed_format=fmt)
            got, n = encoded(res)
            assert n == want.size and np.array_equal(got, want), (kind, fmt)
            back = codec.decode(res, output=fmt)
            assert back.dtype == torch.uint8 and tuple(back.shape) == (w * h * 3 // 2,) and np.array_equal(host(back), payload), (kind, fmt)
            assert np.array_equal(host(codec.decode(res)), x), (kind, fmt)
    # samples above 4095 saturate as tdk_encode12_u16 has it; for the standard order the bytes are that kernel's
    x, stream = reference('uniform', w, h, 16)
    data = upload(stream, dev)
    for fmt, ids in ((td.PackedFormat.Packed12, False), (td.PackedFormat.Packed12_IDS, True)):
        assert np.array_equal(host(td.RawCodec(dev, (w, h), bits=16).decode(data, output=fmt)), spec.pack12(x, ids)), fmt
    assert torch.equal(codec.decode(data, output=td.PackedFormat.Packed12), td.encode12_u16(upload(x, dev).reshape(-1)))


def test_packed_odd_width_next_to_a_refused_segment(td, dev):
    """A pair that reaches into a segment the decoder refuses: both of its writers-to-be agree on zeros for that segment's sample.  The
    altered width claims 17 words of a constant frame's empty payload: they lie inside the tensor of max_stream_bytes."""
    w, h = 513, 2
    spans = spec.geometry(w, h)[0]
    codec = td.RawCodec(dev, (w, h))
    flat, stream = reference('constant', w, h)
    at_widths = spec.sections(w, h)[2]
    for row, span in ((1, 0), (1, 8), (0, 8)):   # the segment a row's last site reaches into; the one a segment's last site does; the reaching one itself
        bad = stream.copy()
        bad[at_widths + 2 * (row * spans + span)] = 17
        want, want_status = spec.decode(bad, w, h)
        assert want_status == spec.BAD_TABLES and want.any() and not want.all()
        buf = torch.zeros(codec.max_stream_bytes(), dtype=torch.uint8, device=dev)
        buf[:bad.size].copy_(torch.from_numpy(bad))
        for fmt, ids in ((td.PackedFormat.Packed12, False), (td.PackedFormat.Packed12_IDS, True)):
            got, status = codec.decode(buf[:bad.size], output=fmt, return_status=True)
            assert int(status.item()) == spec.BAD_TABLES and np.array_equal(host(got), spec.pack12(want, ids)), (row, span, fmt)


def test_small_out_buffer(td, dev):
    w, h = 1030, 5
    codec = td.RawCodec(dev, (w, h))
    x, want = reference('ramp', w, h)
    xs = upload(x, dev)
    tables, need = codec.table_bytes(), want.size
    assert tables + 64 < need
    for capacity in (tables, tables + 4, (tables + need) // 2 // 4 * 4, need - 4, need - 1):
        buf = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=dev)
        res = codec.encode(xs, out=buf[:capacity])
        assert int(res.length.item()) == -1, capacity
        assert bool((buf[capacity:] == GUARD).all()), capacity
        assert np.array_equal(host(buf[:tables])[:16], want[:16])   # the tables always fit; the header tells the true need
        assert spec.parse_header(host(buf[:32]))[5] == need
        with pytest.raises(RuntimeError, match='does not fit'):
            res.to_host()
    buf = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=dev)
    res = codec.encode(xs, out=buf[:need])   # exactly the need
    assert int(res.length.item()) == need and np.array_equal(host(buf[:need]), want) and bool((buf[need:] == GUARD).all())
    assert np.array_equal(res.to_host().numpy(), want)
    got = td.rawcodec.retrieve([res, codec.encode(xs)])
    assert len(got) == 2 and all(np.array_equal(g.numpy(), want) for g in got)
    with pytest.raises(RuntimeError, match='capacity'):   # below the tables: refused on the host
        td._native.check(td._native.lib.tdk_rawcodec_encode(xs.data_ptr(), spec.U16, w, h, 12, buf.data_ptr(), tables - 1, res.length.data_ptr(), None))


@pytest.mark.parametrize('w', [700, 1024])   # rows of 11 spans; whole segments, which the checking workgroup reads 16 bytes at a time
def test_status_bits(td, dev, w):
    h = 4
    spans = spec.geometry(w, h)[0]
    codec = td.RawCodec(dev, (w, h))
    x, stream = reference('ramp', w, h)
    room = codec.max_stream_bytes()
    at_anchors, at_offsets, at_widths, at_payload = spec.sections(w, h)

    def run(data_host, data_bytes):
        """The stream in the head of a tensor of max_stream_bytes (zeros behind it); the decoder is told data_bytes."""
        buf = torch.zeros(room, dtype=torch.uint8, device=dev)
        buf[:data_host.size].copy_(torch.from_numpy(np.array(data_host)))
        out = torch.full((h, w), 0x5A5A, dtype=torch.int16, device=dev).view(torch.uint16)
        got, status = codec.decode(buf[:data_bytes], out=out, return_status=True)
        assert got is out
        want, want_status = spec.decode(host(buf[:data_bytes]), w, h)
        assert int(status.item()) == want_status and np.array_equal(host(got), want)
        return want_status, want

    def altered(at, fmt, value, base=stream):
        out = base.copy()
        out[at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
        return out

    assert run(stream, stream.size)[0] == 0
    assert run(stream, room)[0] == 0                                       # bytes behind the stream do no harm
    for bad in (altered(0, '<I', 0x12345678), altered(4, '<H', 2)):
        status, want = run(bad, stream.size)
        assert status == codec.BAD_MAGIC and not want.any()
    for bad in (altered(8, '<I', w + 2), altered(12, '<I', h + 1)):
        status, want = run(bad, stream.size)
        assert status == codec.BAD_SIZE and not want.any()
    status, want = run(altered(8, '<I', w + 2, altered(0, '<I', 0)), stream.size)
    assert status == codec.BAD_MAGIC | codec.BAD_SIZE and not want.any()
    # bit 2 -- one offset behind the stream's end (but inside the tensor): that segment alone is zero
    far = (room - at_payload) // 4 - 300
    assert at_payload + 4 * far > stream.size
    status, want = run(altered(at_offsets + 4 * 5, '<I', far), stream.size)
    assert status == codec.BAD_TABLES and not want[2, 512:].any() and np.array_equal(want[:2], x[:2]) and np.array_equal(want[2, :512], x[2, :512])
    # ... the payload of the last segments cut off, then the tables themselves
    status, want = run(stream, stream.size - 8)
    assert status == codec.BAD_TABLES and not want[3, 512:].any() and np.array_equal(want[:3], x[:3])
    status, want = run(stream, at_payload - 4)
    assert status == codec.BAD_TABLES and not want.any()
    status, want = run(stream, 32)
    assert status == codec.BAD_TABLES and not want.any()
    # ... a width byte above 16, in a constant frame: the 17 words it claims lie inside the tensor and inside the wave's staging room
    flat, flat_stream = reference('constant', w, h)
    status, want = run(altered(at_widths + 2 * (spans + 3) + 1, '<B', 17, flat_stream), flat_stream.size)
    assert status == codec.BAD_TABLES and not want[1, :512].any() and np.array_equal(want[0], flat[0]) and np.array_equal(want[1, 512:], flat[1, 512:])
    status, want = run(altered(at_widths + 2 * (spans + 3) + 1, '<B', 17, flat_stream), room)   # the same with room for the words: still refused
    assert status == codec.BAD_TABLES and not want[1, :512].any()
    status, want = run(altered(at_widths + 2 * (spans + 3) + 1, '<B', 16, flat_stream), room)   # 16 is a width: zeros behind the stream decode as no change
    assert status == 0 and np.array_equal(want, flat)


def test_offset_views(td, dev):
    w, h = 130, 5
    codec = td.RawCodec(dev, (w, h))
    x, want = reference('ramp', w, h, 12, twelve=True)
    room = codec.max_stream_bytes()
    for offset in (1, 2, 3):   # the frame starts at an odd or an even element; the stream buffer at any multiple of 4 bytes
        buf = torch.full((room + 64,), GUARD, dtype=torch.uint8, device=dev)
        res = codec.encode(upload(x, dev, offset), out=buf[4 * offset:4 * offset + room])
        got, n = encoded(res)
        assert n == want.size and np.array_equal(got, want), offset
        assert bool((buf[:4 * offset] == GUARD).all()) and bool((buf[4 * offset + n:] == GUARD).all()), offset
        for ids, fmt in ((False, td.PackedFormat.Packed12), (True, td.PackedFormat.Packed12_IDS)):
            payload = spec.pack12(x, ids)
            got, n = encoded(codec.encode(upload(payload, dev, offset), packed_format=fmt))
            assert n == want.size and np.array_equal(got, want), (offset, fmt)
            outbuf = torch.full((payload.size + offset + 8,), GUARD, dtype=torch.uint8, device=dev)
            back = codec.decode(res, output=fmt, out=outbuf[offset:])   # longer than the frame: what lies behind it is left alone
            assert np.array_equal(host(back[:payload.size]), payload) and bool((outbuf[:offset] == GUARD).all()) and bool((outbuf[offset + payload.size:] == GUARD).all())
        for output, expected in ((torch.uint16, x), (torch.float32, spec.to_float32(x)), (torch.float16, spec.to_float16(x))):
            outbuf = torch.zeros((w * h + offset + 4) * expected.itemsize, dtype=torch.uint8, device=dev).view(output)
            back = codec.decode(res, output=output, out=outbuf[offset:offset + w * h].view(h, w))
            assert np.array_equal(bits(host(back)), bits(expected)), (offset, output)
            assert not host(outbuf[:offset]).any() and not host(outbuf[offset + w * h:]).any(), (offset, output)
    with pytest.raises(RuntimeError, match='alignment'):   # a stream buffer must start at a multiple of 4 bytes
        codec.encode(upload(x, dev), out=torch.empty(room + 8, dtype=torch.uint8, device=dev)[2:])


def test_second_stream_and_graph_capture(td, dev):
    w, h = 514, 5
    codec = td.RawCodec(dev, (w, h))
    x, want = reference('ramp', w, h)
    other, other_want = reference('outlier', w, h)
    xs = upload(x, dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        res = codec.encode(xs)
        back = codec.decode(res)
    stream.synchronize()
    assert res.stream == stream
    got, n = encoded(res)
    assert n == want.size and np.array_equal(got, want) and np.array_equal(host(back), x)
    assert np.array_equal(res.to_host().numpy(), want)   # from the default stream: waits for the encode's

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):   # capturable from the first call of this object: nothing of it ran before
            fresh = td.RawCodec(dev, (w, h))
            captured = fresh.encode(xs)
            decoded, status = fresh.decode(captured, return_status=True)
            mosaic = fresh.decode(captured, output=torch.float32)
    torch.cuda.synchronize()
    for frame_, stream_ in ((other, other_want), (x, want)):   # the captured calls follow the input tensor as it is at the replay
        xs.copy_(torch.from_numpy(np.array(frame_)))
        graph.replay()
        torch.cuda.synchronize()
        got, n = encoded(captured)
        assert n == stream_.size and np.array_equal(got, stream_)
        assert int(status.item()) == 0 and np.array_equal(host(decoded), frame_)
        assert np.array_equal(bits(host(mosaic)), bits(spec.to_float32(frame_)))


@pytest.mark.parametrize('padding,fmt', [(0, 'Packed12'), (16, 'Packed12_IDS')])
def test_process_compressed_is_process_on_the_packed_bytes(td, dev, padding, fmt):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor
    from torch_darktable.synthetic import synthetic_bayer

    w, h = 64, 48
    fmt = getattr(td.PackedFormat, fmt)
    ids = fmt is td.PackedFormat.Packed12_IDS
    mosaic = (synthetic_bayer(h, w, seed=21, device='cpu', noise_sigma=0.01).clamp(0.0, 1.0) * 4095.0).round().numpy().astype(np.uint16).reshape(h, w)
    payload = np.concatenate([spec.pack12(mosaic, ids), np.arange(1, padding + 1, dtype=np.uint8)])
    make = lambda: ImageProcessor((w, h), td.BayerPattern.RGGB, fmt, ImageProcessingSettings(), dev, None, padding=padding)
    packed_proc, compressed_proc, codec = make(), make(), td.RawCodec(dev, (w, h))
    assert packed_proc.expected_bytes == payload.size
    packed = upload(payload, dev)
    res = codec.encode(packed[:payload.size - padding], packed_format=fmt)
    assert np.array_equal(res.to_host().numpy(), spec.encode(mosaic))
    buffer, _ = compressed_proc._decompress(res, codec)
    assert buffer.numel() == payload.size and np.array_equal(host(buffer[:payload.size - padding]), payload[:payload.size - padding])
    assert not buffer[payload.size - padding:].any()   # the padding bytes are zero
    for step in range(2):   # the second call: the moving averages of bounds and metrics
        want = packed_proc.process(packed, 'cam')
        got = compressed_proc.process_compressed(res if step == 0 else res.data[:int(res.length.item())], 'cam', codec)
        assert got.dtype == torch.uint8 and torch.equal(got, want), step
        assert list(compressed_proc.compressed_status) == ['cam'] and int(compressed_proc.compressed_status['cam'].item()) == 0
    sets = compressed_proc.process_image_set_compressed({'a': res, 'b': res}, codec)
    both = packed_proc.process_image_set({'a': packed, 'b': packed})
    assert list(sets) == ['a', 'b'] and all(torch.equal(sets[k], both[k]) for k in sets)
    assert list(compressed_proc.compressed_status) == ['a', 'b']
    # a truncated stream goes through as a black frame: the status of the call says so
    compressed_proc.process_compressed(res.data[:codec.table_bytes()], 'cam', codec)
    assert int(compressed_proc.compressed_status['cam'].item()) == codec.BAD_TABLES
