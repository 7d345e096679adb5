"""CPU-only: the NumPy restatement of the raw codec (tests/rawcodec_spec.py) against itself -- the vectorised encoder and decoder the
GPU tests compare the kernels with are held to literal per-sample loops on small frames, every content class survives the round trip,
and the sizes the format promises (a constant frame is exactly the tables, an alternation of 0 and 0x8000 fills every full group with
16 planes, a noisy 12-bit ramp comes out smaller than its packed form) hold."""

import struct

import numpy as np
import pytest

import rawcodec_spec as spec

SMALL = [(1, 1), (2, 1), (1, 3), (63, 2), (64, 1), (65, 2), (130, 1), (511, 1), (512, 2), (513, 1), (1030, 2)]


def test_sizes():
    assert spec.geometry(1, 1) == (1, 1) and spec.geometry(64, 5) == (1, 1) and spec.geometry(65, 5) == (2, 1) and spec.geometry(513, 5) == (9, 2)
    assert spec.table_bytes(1, 1) == 32 + 8 + 4 and spec.table_bytes(64, 2) == 32 + 16 + 4 and spec.table_bytes(1030, 5) == 32 + 8 * 5 * 3 + 172
    assert spec.max_stream_bytes(64, 2) == spec.table_bytes(64, 2) + 4 * 32 * 2
    assert spec.table_bytes(4096, 3072) * 8 / (4096 * 3072) == pytest.approx(0.375, abs=1e-4)   # the overhead the header states
    assert spec.sections(1030, 5) == (32, 32 + 60, 32 + 120, spec.table_bytes(1030, 5))


def test_zigzag():
    d = np.array([0, 0xFFFF, 1, 0xFFFE, 2, 0x8000, 0x7FFF])
    assert spec.zigzag(d).tolist() == [0, 1, 2, 3, 4, 0xFFFF, 0xFFFE]
    every = np.arange(65536)
    assert sorted(spec.zigzag(every).tolist()) == every.tolist() and (spec.unzigzag(spec.zigzag(every)) == every).all()
    assert spec.bit_length(np.array([0, 1, 2, 3, 255, 256, 65535])).tolist() == [0, 1, 2, 2, 8, 9, 16]


@pytest.mark.parametrize('kind', spec.CLASSES)
def test_vectorised_forms_are_the_loops(kind):
    for width, height in SMALL:
        frame = spec.frame(kind, width, height)
        stream = spec.encode(frame, bits=16)
        assert stream.tobytes() == spec.encode_loops(frame, bits=16).tobytes(), (kind, width, height)
        decoded, status = spec.decode(stream, width, height)
        assert status == 0 and (decoded == frame).all() and (spec.decode_loops(stream, width, height) == frame).all(), (kind, width, height)


@pytest.mark.parametrize('kind', spec.CLASSES)
def test_round_trip_and_header(kind):
    width, height = 1100, 37
    frame = spec.frame(kind, width, height)
    stream = spec.encode(frame, bits=14)
    version, bits, w, h, payload_words, total_bytes, flags, reserved = spec.parse_header(stream)
    assert (version, bits, w, h, flags, reserved) == (1, 14, width, height, 0, 0)
    assert total_bytes == stream.size == spec.table_bytes(width, height) + 4 * payload_words <= spec.max_stream_bytes(width, height)
    decoded, status = spec.decode(stream, width, height)
    assert status == 0 and decoded.dtype == np.uint16 and (decoded == frame).all()
    _, at_offsets, at_widths, at_payload = spec.sections(width, height)
    offsets = stream[at_offsets:at_widths].view('<u4')
    assert offsets[0] == 0 and (np.diff(offsets.astype(np.int64)) >= 0).all() and offsets[-1] <= payload_words
    assert stream[at_widths:at_payload].max() <= 16


def test_constant_frame_is_exactly_the_tables():
    for width, height in SMALL + [(4096, 8)]:
        stream = spec.encode(spec.frame('constant', width, height))
        assert stream.size == spec.table_bytes(width, height), (width, height)
        anchors = stream[spec.sections(width, height)[0]:spec.sections(width, height)[1]].view('<u2')
        assert set(anchors.tolist()) <= {0, 1234}


def test_alternation_fills_every_full_group():
    width, height = 1030, 3
    stream = spec.encode(spec.frame('alternating', width, height))
    s, _ = spec.geometry(width, height)
    _, _, at_widths, _ = spec.sections(width, height)
    widths = stream[at_widths:at_widths + 2 * height * s].reshape(height, s, 2)
    full = width // 64
    assert (widths[:, :full] == 16).all()
    assert (widths[:, full:] == [[16, 16]]).all()   # the last span holds sites 1024..1029: three samples of each parity, two differences
    # a span of one site per parity at the head of a segment has nothing but the anchor
    lone = spec.encode(spec.frame('alternating', 1026, 1))
    assert lone[spec.sections(1026, 1)[2]:][2 * 16:2 * 16 + 2].tolist() == [0, 0]


def test_noisy_ramp_is_smaller_than_packed():
    width, height = 2048, 64
    for a, b in ((2e-5, 1e-6), (1e-4, 4e-6), (4e-4, 1e-5)):
        frame = spec.noisy_ramp(width, height, a, b)
        stream = spec.encode(frame)
        packed = width * height * 3 // 2
        print(f'a={a} b={b}: {8 * stream.size / (width * height):.2f} bits per site, {packed / stream.size:.2f} x against packed 12')
        assert stream.size < packed
        assert (spec.decode(stream, width, height)[0] == frame).all()


def test_decode_reports_what_is_wrong():
    width, height = 700, 4
    frame = spec.frame('ramp', width, height)
    stream = spec.encode(frame)
    at_anchors, at_offsets, at_widths, at_payload = spec.sections(width, height)
    zero = np.zeros_like(frame)

    def altered(at, fmt, value):
        out = stream.copy()
        out[at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
        return out

    for bad in (altered(0, '<I', 0x12345678), altered(4, '<H', 2)):
        decoded, status = spec.decode(bad, width, height)
        assert status == spec.BAD_MAGIC and (decoded == zero).all()
    for bad in (altered(8, '<I', width + 1), altered(12, '<I', height - 1)):
        decoded, status = spec.decode(bad, width, height)
        assert status == spec.BAD_SIZE and (decoded == zero).all()
    decoded, status = spec.decode(stream, width, height + 1)
    assert status == spec.BAD_SIZE and decoded.shape == (height + 1, width) and not decoded.any()
    # one offset past the end: that segment alone is zero (segment 1 of row 2: sites 512..699)
    decoded, status = spec.decode(altered(at_offsets + 4 * 5, '<I', stream.size), width, height)
    expected = frame.copy()
    expected[2, 512:] = 0
    assert status == spec.BAD_TABLES and (decoded == expected).all()
    # a width byte above 16: span 3 of row 1 belongs to segment 0 of that row
    decoded, status = spec.decode(altered(at_widths + 2 * (11 + 3), '<B', 17), width, height)
    expected = frame.copy()
    expected[1, :512] = 0
    assert status == spec.BAD_TABLES and (decoded == expected).all()
    # a truncated stream: the segments whose payload is cut are zero, the ones in front of the cut are intact
    decoded, status = spec.decode(stream[:stream.size - 4], width, height)
    expected = frame.copy()
    expected[3, 512:] = 0
    assert status == spec.BAD_TABLES and (decoded == expected).all()
    decoded, status = spec.decode(stream[:at_payload - 1], width, height)
    assert status == spec.BAD_TABLES and not decoded.any()


def test_packed_and_float_forms():
    samples = np.array([0, 1, 4095, 4096, 65535, 0x0ABC, 0x0123, 2048], dtype=np.uint16)
    for ids in (False, True):
        packed = spec.pack12(samples, ids)
        assert packed.size == 12
        assert spec.unpack12(packed, ids).tolist() == np.minimum(samples, 4095).tolist()
    assert spec.pack12(np.array([0x0ABC, 0x0123]), False).tolist() == [0xBC, 0x3A, 0x12]
    assert spec.pack12(np.array([0x0ABC, 0x0123]), True).tolist() == [0xAB, 0x12, 0x3C]
    assert spec.to_float32(samples).dtype == np.float32 and spec.to_float32(samples)[2] == np.float32(4095) * np.float32(1.0 / 4095.0)
    assert spec.to_float16(samples).dtype == np.float16
