"""Lossless compression of raw mosaics on the device (include/tdk_hip_rawcodec.h, the normative text of the format "TDKR").

A raw frame moves as 1.5 bytes a site in the packed container; the host link and the disk are by now as large as the kernels.  `RawCodec`
encodes a mosaic -- uint16 codes, or packed 12-bit bytes in either nibble order -- into a self-describing byte stream and decodes it
again, both on the device; every uint16 value survives.  The format needs no Bayer pattern: same-colour neighbours are two sites apart
in a row, a sample is predicted by the one before it, and the differences of 32 samples are stored as bit planes of their common width.

    codec = RawCodec(device, (4096, 3072))
    res = codec.encode(mosaic_u16)                   # returns at once: res.data and res.length stay on the device
    data = res.to_host()                             # synchronises: a CPU uint8 tensor of the stream's length
    frame = codec.decode(data.to(device))            # (H, W) uint16
    mosaic = codec.decode(res, output=torch.float32) # the bits of decode12_float on the same samples
    packed = codec.decode(res, output=PackedFormat.Packed12)

`encode` is three launches and `decode` one, on PyTorch's current stream: no workspace, no atomics on global memory, no memset, no copy,
no synchronisation, so both can be captured in a graph from the first call.  The stream's length and the decoder's status stay in
device memory.  There is no CPU fallback."""

from __future__ import annotations

import struct

import torch

from ._frames import require_cuda_device
from ._native import (TDK_RAW_F16, TDK_RAW_F32, TDK_RAW_PACKED12, TDK_RAW_PACKED12_IDS, TDK_RAW_U16, TDK_RAWCODEC_BAD_MAGIC, TDK_RAWCODEC_BAD_SIZE, TDK_RAWCODEC_BAD_TABLES,
                      TDK_RAWCODEC_FORMAT_VERSION, TDK_RAWCODEC_HEADER_BYTES, TDK_RAWCODEC_MAX_SITES, check, lib)
from .bayer import PackedFormat
from .torch_darktable_extension import _ptr, _require, _stream

_PACKED = {PackedFormat.Packed12: TDK_RAW_PACKED12, PackedFormat.Packed12_IDS: TDK_RAW_PACKED12_IDS}
_OUTPUTS = {torch.uint16: TDK_RAW_U16, torch.float32: TDK_RAW_F32, torch.float16: TDK_RAW_F16, **_PACKED}
_MAGIC = b'TDKR'


class RawCodecResult:
    """One encode: `data` is the stream's buffer (1-D uint8 on the device), `length` a 0-dim int64 on the device: the stream's length,
    or -1 when it did not fit in `data`.  Both are final once the stream the encode was issued on has got there."""

    def __init__(self, data: torch.Tensor, length: torch.Tensor, stream: torch.cuda.Stream):
        self.data, self.length, self.stream = data, length, stream

    def _wait(self) -> torch.cuda.Stream:
        here = torch.cuda.current_stream(self.data.device)
        here.wait_stream(self.stream)
        return here

    def to_host(self) -> torch.Tensor:
        """The stream as a CPU uint8 tensor (synchronises); RuntimeError if it did not fit in `data`."""
        with torch.cuda.device(self.data.device):
            self._wait()
            n = int(self.length.item())
            _check_length(n, self.data)
            return self.data[:n].cpu()


def _check_length(n: int, data: torch.Tensor) -> None:
    if n < 0:
        raise RuntimeError(f'RawCodec: the stream does not fit in the output buffer ({data.numel()} bytes)')


def retrieve(results) -> list:
    """The host byte streams of several encodes: every length crosses in one synchronisation, then the bytes in a second."""
    results = list(results)
    if not results:
        return []
    dev = results[0].data.device
    with torch.cuda.device(dev):
        for r in results:
            here = r._wait()
        lengths = torch.stack([r.length for r in results]).cpu().tolist()
        for r, n in zip(results, lengths):
            _check_length(n, r.data)
        out = [r.data[:n].to('cpu', non_blocking=True) for r, n in zip(results, lengths)]
        here.synchronize()
    return out


class RawCodec:
    """The codec of one frame size; image_size is (width, height), 1..65535 each and at most 2^30 sites.  `bits` (1..16) is written
    into the header for the reader's information and changes nothing else: every uint16 value is kept whatever it says.  The packed
    forms need an even number of sites and bits = 12."""

    BAD_MAGIC, BAD_SIZE, BAD_TABLES = TDK_RAWCODEC_BAD_MAGIC, TDK_RAWCODEC_BAD_SIZE, TDK_RAWCODEC_BAD_TABLES   # bits of the decoder's status

    def __init__(self, device: torch.device, image_size: tuple[int, int], bits: int = 12):
        require_cuda_device(device)
        width, height = (int(v) for v in image_size)
        self._check_size(width, height)
        if isinstance(bits, bool) or int(bits) != bits or not 1 <= int(bits) <= 16:
            raise ValueError(f'bits must be an integer in 1..16, got {bits}')
        self._device = device
        self.width, self.height, self.bits = width, height, int(bits)

    @staticmethod
    def _check_size(width: int, height: int) -> None:
        if not (1 <= width <= 65535 and 1 <= height <= 65535 and width * height <= TDK_RAWCODEC_MAX_SITES):
            raise ValueError(f'Image dimensions must be 1..65535 with at most 2^30 sites, got {width}x{height}')

    @property
    def image_size(self) -> tuple[int, int]:
        return (self.width, self.height)

    def __repr__(self):
        return f'RawCodec({self.width}x{self.height}, bits={self.bits})'

    def table_bytes(self) -> int:
        """Header, anchors, offsets and widths: the length of the stream of a constant frame."""
        return int(lib.tdk_rawcodec_table_bytes(self.width, self.height))

    def max_stream_bytes(self) -> int:
        """A capacity every stream of this size fits in."""
        return int(lib.tdk_rawcodec_max_stream_bytes(self.width, self.height))

    def packed_bytes(self) -> int:
        """The bytes of the frame in a packed 12-bit container."""
        return self.width * self.height * 3 // 2

    def _packed_tag(self, packed_format) -> int:
        if packed_format not in _PACKED:
            raise ValueError(f'packed_format must be PackedFormat.Packed12 or PackedFormat.Packed12_IDS, got {packed_format!r}')
        if (self.width * self.height) % 2:
            raise ValueError(f'A packed frame needs an even number of sites, got {self.width}x{self.height}')
        return _PACKED[packed_format]

    def encode(self, frame: torch.Tensor, out: torch.Tensor | None = None, packed_format: PackedFormat | None = None) -> RawCodecResult:
        """Enqueue the encode of `frame` on the current stream: an (H, W) uint16 tensor, or with `packed_format` the 1-D uint8 tensor of
        its packed 12-bit bytes (the samples are those of decode12_u16).  `out`: a contiguous 1-D uint8 buffer on the frame's device for
        the stream, at least table_bytes() long and 4-byte aligned (default: a new one of max_stream_bytes()).  When the stream does
        not fit, `length` is -1 and nothing behind `out` is touched."""
        if not isinstance(frame, torch.Tensor):
            raise TypeError(f'frame must be a tensor, got {type(frame).__name__}')
        if packed_format is None:
            if frame.dtype != torch.uint16 or tuple(frame.shape) != (self.height, self.width):
                raise RuntimeError(f'RawCodec input {tuple(frame.shape)} {frame.dtype} != expected {(self.height, self.width)} torch.uint16 '
                                   '(packed bytes take packed_format=)')
            tag, bits = TDK_RAW_U16, self.bits
        else:
            tag, bits = self._packed_tag(packed_format), 12
            if self.bits != 12:
                raise ValueError(f'A packed frame holds 12 bits, the codec was built with bits={self.bits}')
            if frame.dtype != torch.uint8 or frame.dim() != 1 or frame.numel() != self.packed_bytes():
                raise RuntimeError(f'RawCodec packed input {tuple(frame.shape)} {frame.dtype} != expected ({self.packed_bytes()},) torch.uint8')
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1:
                raise ValueError('out must be a 1-D uint8 tensor')
            if out.numel() < self.table_bytes():
                raise ValueError(f'out holds {out.numel()} bytes, the tables alone take {self.table_bytes()}')
        _require(frame.is_cuda, 'Input must be on CUDA device')
        _require(frame.is_contiguous(), 'Input must be contiguous')
        if out is not None:
            _require(out.device == frame.device, 'out must be on the device of the input')
            _require(out.is_contiguous(), 'out must be contiguous')
        with torch.cuda.device(frame.device):
            stream = torch.cuda.current_stream(frame.device)
            if out is None:
                out = torch.empty(self.max_stream_bytes(), dtype=torch.uint8, device=frame.device)
            length = torch.empty((), dtype=torch.int64, device=frame.device)
            rc = lib.tdk_rawcodec_encode(_ptr(frame), tag, self.width, self.height, bits, _ptr(out), out.numel(), _ptr(length), _stream())
        check(rc)
        return RawCodecResult(out, length, stream)

    def _output(self, output):
        if output not in _OUTPUTS:
            raise ValueError(f'output must be torch.uint16, torch.float32, torch.float16 or a PackedFormat, got {output!r}')
        if output in _PACKED:
            self._packed_tag(output)
            return _OUTPUTS[output], torch.uint8, (self.packed_bytes(),)
        return _OUTPUTS[output], output, (self.height, self.width)

    def decode(self, stream, output=torch.uint16, out: torch.Tensor | None = None, return_status: bool = False):
        """Enqueue the decode of `stream` on the current stream: a RawCodecResult, or a 1-D uint8 device tensor whose whole length is
        the stream (4-byte aligned).  output: torch.uint16 -> (H, W) codes; torch.float32 / torch.float16 -> the mosaic decode12_float /
        decode12_half give on the same samples; PackedFormat.* -> the packed 12-bit bytes (a sample above 4095 becomes 4095).  `out`: a
        contiguous tensor of that type and shape; for a packed output any 1-D uint8 buffer at least as long (bytes behind the frame
        are left alone).  return_status: also the decoder's status, a 0-dim int32 device tensor -- 0, or BAD_MAGIC | BAD_SIZE (the
        output is zero) or BAD_TABLES (the offending segments are zero).  Nothing outside the two buffers is touched whatever the
        stream holds."""
        tag, dtype, shape = self._output(output)
        data = stream.data if isinstance(stream, RawCodecResult) else stream
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError('stream must be a RawCodecResult or a 1-D uint8 tensor')
        if data.numel() < TDK_RAWCODEC_HEADER_BYTES:
            raise ValueError(f'stream holds {data.numel()} bytes, a header alone takes {TDK_RAWCODEC_HEADER_BYTES}')
        if out is not None:
            fits = isinstance(out, torch.Tensor) and out.dtype == dtype
            fits = fits and ((out.dim() == 1 and out.numel() >= shape[0]) if output in _PACKED else tuple(out.shape) == shape)
            if not fits:
                raise ValueError(f'out must be a {dtype} tensor of shape {shape}' + (' or longer' if output in _PACKED else ''))
        _require(data.is_cuda, 'Input must be on CUDA device')
        _require(data.is_contiguous(), 'Input must be contiguous')
        if out is not None:
            _require(out.device == data.device, 'out must be on the device of the input')
            _require(out.is_contiguous(), 'out must be contiguous')
        with torch.cuda.device(data.device):
            if isinstance(stream, RawCodecResult):
                stream._wait()
            if out is None:
                out = torch.empty(shape, dtype=dtype, device=data.device)
            status = torch.empty((), dtype=torch.int32, device=data.device)
            rc = lib.tdk_rawcodec_decode(_ptr(data), data.numel(), _ptr(out), tag, self.width, self.height, _ptr(status), _stream())
        check(rc)
        return (out, status) if return_status else out

    @staticmethod
    def parse_header(data) -> dict:
        """The header of a stream read from disk (bytes, bytearray, or a uint8 tensor; on the host): a dict of version, bits, width,
        height, payload_words, total_bytes, flags.  ValueError on a short buffer, a wrong magic or version, or sizes that contradict
        each other."""
        if isinstance(data, torch.Tensor):
            if data.dtype != torch.uint8 or data.dim() != 1:
                raise ValueError('stream must be bytes or a 1-D uint8 tensor')
            raw = bytes(data[:TDK_RAWCODEC_HEADER_BYTES].cpu().tolist())
        else:
            raw = bytes(data[:TDK_RAWCODEC_HEADER_BYTES])
        if len(raw) < TDK_RAWCODEC_HEADER_BYTES:
            raise ValueError(f'A TDKR stream starts with a header of {TDK_RAWCODEC_HEADER_BYTES} bytes, got {len(raw)}')
        if raw[:4] != _MAGIC:
            raise ValueError(f'Not a TDKR stream: magic {raw[:4]!r}')
        version, bits, width, height, payload_words, total_bytes, flags, _ = struct.unpack('<HHIIIIII', raw[4:])
        if version != TDK_RAWCODEC_FORMAT_VERSION:
            raise ValueError(f'TDKR version {version} is not supported (this package reads version {TDK_RAWCODEC_FORMAT_VERSION})')
        if not (1 <= width <= 65535 and 1 <= height <= 65535 and width * height <= TDK_RAWCODEC_MAX_SITES):
            raise ValueError(f'TDKR header: frame size {width}x{height} outside 1..65535 or above 2^30 sites')
        tables = int(lib.tdk_rawcodec_table_bytes(width, height))
        if total_bytes != tables + 4 * payload_words or total_bytes > int(lib.tdk_rawcodec_max_stream_bytes(width, height)):
            raise ValueError(f'TDKR header: total_bytes {total_bytes} does not match {tables} bytes of tables and {payload_words} payload words')
        return {'version': version, 'bits': bits, 'width': width, 'height': height, 'payload_words': payload_words, 'total_bytes': total_bytes, 'flags': flags}


__all__ = ['RawCodec', 'RawCodecResult']
