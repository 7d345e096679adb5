"""CPU-only: the header include/tdk_hip_rawcodec.h (the lossless raw codec) -- it parses to exactly its five declarations (exports and
the ctypes table: tests/test_header_abi.py), every argument error of tdk_rawcodec_encode and tdk_rawcodec_decode is reported on the host
before any HIP call, the size queries give what the NumPy restatement gives, and the Python front-end torch_darktable.RawCodec and the
two pipeline methods exist and validate their arguments without a device."""

import inspect
import re
import struct
from pathlib import Path

import pytest

import rawcodec_spec as spec
from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_rawcodec.h'
EXPECTED = ['tdk_rawcodec_abi_version', 'tdk_rawcodec_decode', 'tdk_rawcodec_encode', 'tdk_rawcodec_max_stream_bytes', 'tdk_rawcodec_table_bytes']
PACKED12, PACKED12_IDS, U16, F32, F16 = 0, 1, 2, 3, 4


def test_header_declares_the_codec_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_RAWCODEC_ABI_VERSION 1', 'TDK_RAWCODEC_FORMAT_VERSION 1', 'TDK_RAWCODEC_HEADER_BYTES 32', 'TDK_RAWCODEC_SPAN 64', 'TDK_RAWCODEC_SEGMENT 512',
                   'TDK_RAWCODEC_MAX_SITES 1073741824', 'TDK_RAWCODEC_BAD_MAGIC 1', 'TDK_RAWCODEC_BAD_SIZE 2', 'TDK_RAWCODEC_BAD_TABLES 4'):
        assert re.search(rf'#define {re.escape(define)}(?!\d)', text), define
    assert '#include "tdk_hip.h"' in text and '#include "tdk_hip_raw.h"' in text and 'extern "C"' in text
    assert decls['tdk_rawcodec_abi_version'] == ('int', [])
    assert decls['tdk_rawcodec_table_bytes'] == ('size_t', ['int width', 'int height'])
    assert decls['tdk_rawcodec_max_stream_bytes'] == ('size_t', ['int width', 'int height'])
    assert decls['tdk_rawcodec_encode'] == ('int', ['const void* src', 'int src_format', 'int width', 'int height', 'int bits', 'void* data', 'size_t capacity',
                                                    'int64_t* length', 'tdk_stream_t stream'])
    assert decls['tdk_rawcodec_decode'] == ('int', ['const void* data', 'size_t data_bytes', 'void* out', 'int out_format', 'int width', 'int height', 'int* status',
                                                    'tdk_stream_t stream'])
    for formula in ('z = ((t << 1) ^ (t >> 15)) & 0xFFFF', 'd_0 = 0; for k >= 1, d_k = (v_k - v_(k-1)) mod 2^16', 'word j carries bit j of z of the group\'s i-th sample in bit i',
                    'table_bytes = 32 + 8*H*G + round4(2*H*S)', 'max_stream_bytes = table_bytes + 4*16*2*H*S', 'u16[H][G][2]', 'u32[H][G]', 'u8[H][S][2]',
                    'v_0 = anchor, v_k = (anchor + t_1 + ... + t_k) mod 2^16', 'b2 = ((p1 & 15) << 4) | (p0 & 15)', 'need an even number of sites', 'Why this shape',
                    'No load or store outside', 'normative text'):
        assert formula in text, formula
    assert (_native.TDK_RAWCODEC_FORMAT_VERSION, _native.TDK_RAWCODEC_HEADER_BYTES, _native.TDK_RAWCODEC_SPAN, _native.TDK_RAWCODEC_SEGMENT) == (
        spec.VERSION, spec.HEADER_BYTES, spec.SPAN, spec.SEGMENT) == (1, 32, 64, 512)
    assert (_native.TDK_RAWCODEC_BAD_MAGIC, _native.TDK_RAWCODEC_BAD_SIZE, _native.TDK_RAWCODEC_BAD_TABLES) == (spec.BAD_MAGIC, spec.BAD_SIZE, spec.BAD_TABLES) == (1, 2, 4)
    assert _native.TDK_RAWCODEC_MAX_SITES == 1 << 30
    assert (_native.TDK_RAW_PACKED12, _native.TDK_RAW_PACKED12_IDS, _native.TDK_RAW_U16, _native.TDK_RAW_F32, _native.TDK_RAW_F16) == (
        spec.PACKED12, spec.PACKED12_IDS, spec.U16, spec.F32, spec.F16)
    assert _native.ABI_VERSIONS['tdk_rawcodec_abi_version'] == (1, 'raw codec ABI')
    assert _native.lib.tdk_rawcodec_abi_version() == 1
    names = [row[0] for row in _native.HEADERS]
    assert names[names.index('tdk_hip_ca.h') + 1] == 'tdk_hip_rawcodec.h'   # directly behind the row of the stage before it
    assert _native.HEADERS[names.index('tdk_hip_rawcodec.h')] == ('tdk_hip_rawcodec.h', _native.RAWCODEC_SIGNATURES, 'tdk_rawcodec_abi_version', 1, 'raw codec ABI')


def test_size_queries_are_the_spec(td):
    from torch_darktable._native import lib

    for width, height in ((1, 1), (2, 1), (64, 2), (65, 3), (511, 7), (512, 7), (513, 7), (1030, 5), (4096, 3072), (8192, 6144), (65535, 3), (3, 65535), (32768, 32768)):
        assert lib.tdk_rawcodec_table_bytes(width, height) == spec.table_bytes(width, height), (width, height)
        assert lib.tdk_rawcodec_max_stream_bytes(width, height) == spec.max_stream_bytes(width, height), (width, height)
    for width, height in ((0, 1), (1, 0), (-4, 4), (65536, 1), (1, 65536), (32768, 32769), (65535, 65535)):
        assert lib.tdk_rawcodec_table_bytes(width, height) == 0 and lib.tdk_rawcodec_max_stream_bytes(width, height) == 0, (width, height)
    assert spec.max_stream_bytes(32768, 32768) < 1 << 32   # total_bytes of the header is a u32


def test_encode_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    w, h = 640, 480
    src, data, length = fake, fake + (1 << 24), fake + (1 << 26)
    capacity = spec.max_stream_bytes(w, h)
    names = ['src', 'src_format', 'width', 'height', 'bits', 'data', 'capacity', 'length', 'stream']

    def rejected(word, **change):
        args = [src, U16, w, h, 12, data, capacity, length, None]
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.tdk_rawcodec_encode(*args) == 1 and word in lib.tdk_last_error() and b'tdk_rawcodec_encode' in lib.tdk_last_error()

    for k in ('src', 'data', 'length'):
        assert rejected(b'null pointer', **{k: None}), k
    for v in (F32, F16, 5, -1):
        assert rejected(b'source format', src_format=v), v
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
    assert rejected(b'frame size', width=32768, height=32769)
    for fmt in (PACKED12, PACKED12_IDS):
        assert rejected(b'even number of sites', src_format=fmt, width=641, height=481)
        assert rejected(b'capacity', src_format=fmt, width=641, capacity=0)   # an odd width alone passes that check: the next refusal speaks
        for v in (11, 16):
            assert rejected(b'bits must be 12', src_format=fmt, bits=v), (fmt, v)
    for v in (0, 17, -1):
        assert rejected(b'bits', bits=v), v
    assert rejected(b'alignment', src=src + 1) and rejected(b'alignment', data=data + 2) and rejected(b'alignment', length=length + 4)
    for v in (0, 31, spec.table_bytes(w, h) - 1):
        assert rejected(b'capacity', capacity=v), v
    assert rejected(b'data overlaps src', data=src + 64) and rejected(b'data overlaps src', src=data + capacity - 2)
    assert rejected(b'length overlaps', length=data + 8) and rejected(b'length overlaps', length=src + w * h * 2 - 8)
    assert rejected(b'data overlaps src', src_format=PACKED12, data=src + w * h * 3 // 2 - 4)   # a packed source is 1.5 bytes a site


def test_decode_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30
    w, h = 640, 480
    data, out, status = fake, fake + (1 << 24), fake + (1 << 26)
    data_bytes = spec.max_stream_bytes(w, h)
    names = ['data', 'data_bytes', 'out', 'out_format', 'width', 'height', 'status', 'stream']

    def rejected(word, **change):
        args = [data, data_bytes, out, U16, w, h, status, None]
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.tdk_rawcodec_decode(*args) == 1 and word in lib.tdk_last_error() and b'tdk_rawcodec_decode' in lib.tdk_last_error()

    for k in ('data', 'out', 'status'):
        assert rejected(b'null pointer', **{k: None}), k
    for v in (5, -1, 17):
        assert rejected(b'output format', out_format=v), v
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
    for fmt in (PACKED12, PACKED12_IDS):
        assert rejected(b'even number of sites', out_format=fmt, width=641, height=481), fmt
    for v in (0, 31):
        assert rejected(b'data_bytes', data_bytes=v), v
    assert rejected(b'alignment', data=data + 2) and rejected(b'alignment', status=status + 2)
    assert rejected(b'alignment', out=out + 1) and rejected(b'alignment', out=out + 2, out_format=F32) and rejected(b'alignment', out=out + 1, out_format=F16)
    assert rejected(b'out overlaps data', out=data + 64) and rejected(b'out overlaps data', data=out + w * h * 2 - 4)
    assert rejected(b'out overlaps data', data=out + w * h * 4 - 4, out_format=F32) and rejected(b'out overlaps data', data=out + w * h * 3 // 2 - 4, out_format=PACKED12)
    assert rejected(b'status overlaps', status=out + 8) and rejected(b'status overlaps', status=data + data_bytes - 4)


def test_package_exports_rawcodec(td):
    import torch
    import torch_darktable

    RC = torch_darktable.RawCodec
    assert RC is torch_darktable.rawcodec.RawCodec and torch_darktable.RawCodecResult is torch_darktable.rawcodec.RawCodecResult
    assert {'RawCodec', 'RawCodecResult', 'rawcodec'} <= set(torch_darktable.__all__)
    assert torch_darktable.rawcodec.__all__ == ['RawCodec', 'RawCodecResult']
    assert callable(torch_darktable.rawcodec.retrieve) and torch_darktable.rawcodec.retrieve([]) == []
    assert (RC.BAD_MAGIC, RC.BAD_SIZE, RC.BAD_TABLES) == (1, 2, 4)
    params = inspect.signature(RC.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bits'] and params['bits'].default == 12
    params = inspect.signature(RC.encode).parameters
    assert list(params) == ['self', 'frame', 'out', 'packed_format'] and [params[k].default for k in ('out', 'packed_format')] == [None, None]
    params = inspect.signature(RC.decode).parameters
    assert list(params) == ['self', 'stream', 'output', 'out', 'return_status']
    assert [params[k].default for k in ('output', 'out', 'return_status')] == [torch.uint16, None, False]
    assert list(inspect.signature(RC.parse_header).parameters) == ['data'] and isinstance(inspect.getattr_static(RC, 'parse_header'), staticmethod)
    assert list(inspect.signature(torch_darktable.RawCodecResult.__init__).parameters) == ['self', 'data', 'length', 'stream']
    assert hasattr(torch_darktable.RawCodecResult, 'to_host')
    assert 'no CPU fallback' in torch_darktable.rawcodec.__doc__


def test_pipeline_has_the_compressed_entry_points(td):
    import torch
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor
    from torch_darktable.pipeline.image_processor import ImageSizeMismatchError

    assert list(inspect.signature(ImageProcessor.process_compressed).parameters) == ['self', 'stream', 'image_name', 'codec']
    assert list(inspect.signature(ImageProcessor.process_image_set_compressed).parameters) == ['self', 'image_set_streams', 'codec']
    # methods only: no constructor slot and no settings field
    assert not {'codec', 'rawcodec', 'compressed'} & set(inspect.signature(ImageProcessor.__init__).parameters)
    for settings in (ImageProcessingSettings, CameraSettings):
        assert not {'codec', 'rawcodec', 'compressed'} & set(settings.model_fields), settings
    dev = torch.device('cuda', 0)
    proc = ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None)
    stream = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(TypeError, match='codec must be a RawCodec'):
        proc.process_compressed(stream, 'a', object())
    with pytest.raises(ImageSizeMismatchError, match='the codec is for'):
        proc.process_compressed(stream, 'a', td.RawCodec(dev, (64, 50)))


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda, cpu = torch.device('cuda', 0), torch.device('cpu')   # a device object only: nothing below needs a GPU
    RC, P = td.RawCodec, td.PackedFormat
    with pytest.raises(ValueError, match='CUDA'):
        RC(cpu, (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48), (32768, 32769)):
        with pytest.raises(ValueError, match='dimensions'):
            RC(cuda, size)
    for bits in (0, 17, 12.5, True):
        with pytest.raises(ValueError, match='bits'):
            RC(cuda, (64, 48), bits=bits)

    codec = RC(cuda, (1030, 5))
    assert codec.image_size == (1030, 5) and codec.bits == 12 and repr(codec) == 'RawCodec(1030x5, bits=12)'
    assert codec.table_bytes() == spec.table_bytes(1030, 5) and codec.max_stream_bytes() == spec.max_stream_bytes(1030, 5) and codec.packed_bytes() == 1030 * 5 * 3 // 2
    frame = torch.zeros(5, 1030, dtype=torch.uint16)
    for wrong in (torch.zeros(1030, 5, dtype=torch.uint16), torch.zeros(5, 1030, dtype=torch.int16), torch.zeros(5 * 1030, dtype=torch.uint16)):
        with pytest.raises(RuntimeError, match='RawCodec input'):
            codec.encode(wrong)
    with pytest.raises(TypeError, match='tensor'):
        codec.encode([[0]])
    packed = torch.zeros(codec.packed_bytes(), dtype=torch.uint8)
    with pytest.raises(ValueError, match='packed_format'):
        codec.encode(packed, packed_format='Packed12')
    with pytest.raises(RuntimeError, match='packed input'):
        codec.encode(packed[:-3], packed_format=P.Packed12)
    with pytest.raises(RuntimeError, match='packed input'):
        codec.encode(frame, packed_format=P.Packed12_IDS)
    with pytest.raises(ValueError, match='even number of sites'):
        RC(cuda, (65, 3)).encode(torch.zeros(291, dtype=torch.uint8), packed_format=P.Packed12)
    with pytest.raises(RuntimeError, match='CUDA'):   # an odd width with an even height is a packed frame like any other
        RC(cuda, (65, 4)).encode(torch.zeros(65 * 6, dtype=torch.uint8), packed_format=P.Packed12)
    with pytest.raises(ValueError, match='12 bits'):
        RC(cuda, (1030, 5), bits=14).encode(packed, packed_format=P.Packed12)
    for out in (torch.zeros(4096, dtype=torch.int8), torch.zeros(4, 1024, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='out must be'):
            codec.encode(frame, out=out)
    with pytest.raises(ValueError, match='the tables alone'):
        codec.encode(frame, out=torch.zeros(codec.table_bytes() - 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='CUDA'):
        codec.encode(frame)   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        codec.encode(packed, packed_format=P.Packed12)

    stream = torch.zeros(codec.max_stream_bytes(), dtype=torch.uint8)
    for output in (torch.int16, torch.uint8, 'uint16', None):
        with pytest.raises(ValueError, match='output must be'):
            codec.decode(stream, output=output)
    with pytest.raises(ValueError, match='even number of sites'):
        RC(cuda, (65, 3)).decode(stream, output=P.Packed12)
    for wrong in (torch.zeros(64, dtype=torch.int32), torch.zeros(2, 64, dtype=torch.uint8), b'TDKR'):
        with pytest.raises(ValueError, match='stream must be'):
            codec.decode(wrong)
    with pytest.raises(ValueError, match='a header alone'):
        codec.decode(stream[:31])
    for output, out in ((torch.uint16, torch.zeros(5, 1030, dtype=torch.float32)), (torch.float32, torch.zeros(1030, 5)), (P.Packed12, torch.zeros(codec.packed_bytes() - 1, dtype=torch.uint8)),
                        (torch.float16, torch.zeros(5, 1030))):
        with pytest.raises(ValueError, match='out must be'):
            codec.decode(stream, output=output, out=out)
    with pytest.raises(RuntimeError, match='CUDA'):
        codec.decode(stream)
    with pytest.raises(RuntimeError, match='CUDA'):
        codec.decode(stream, output=P.Packed12_IDS, out=torch.zeros(codec.packed_bytes() + 16, dtype=torch.uint8))


def test_parse_header_on_the_host(td):
    import numpy as np
    import torch

    RC = td.RawCodec
    stream = spec.encode(spec.frame('ramp', 130, 3), bits=12)
    expected = {'version': 1, 'bits': 12, 'width': 130, 'height': 3, 'payload_words': (stream.size - spec.table_bytes(130, 3)) // 4, 'total_bytes': stream.size, 'flags': 0}
    assert RC.parse_header(stream.tobytes()) == expected and RC.parse_header(torch.from_numpy(stream)) == expected and RC.parse_header(bytearray(stream.tobytes()[:32])) == expected

    def altered(at, fmt, value):
        out = stream.copy()
        out[at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
        return out.tobytes()

    with pytest.raises(ValueError, match='header of 32 bytes'):
        RC.parse_header(stream.tobytes()[:31])
    with pytest.raises(ValueError, match='magic'):
        RC.parse_header(altered(0, '<I', 0x12345678))
    with pytest.raises(ValueError, match='version 2'):
        RC.parse_header(altered(4, '<H', 2))
    for at, value in ((8, 0), (8, 65536), (12, 0)):
        with pytest.raises(ValueError, match='frame size'):
            RC.parse_header(altered(at, '<I', value))
    for at, value in ((16, 5), (20, stream.size + 4), (8, 700)):
        with pytest.raises(ValueError, match='total_bytes'):
            RC.parse_header(altered(at, '<I', value))
    with pytest.raises(ValueError, match='stream must be'):
        RC.parse_header(torch.zeros(64, dtype=torch.int32))
