"""Device-resident JPEG encode (include/tdk_hip_ext.h: tdk_jpeg_encode_device).

The encoder of `Jpeg.encode` with the optimal Huffman tables and the markers built on the device: the byte stream stays in device
memory and its length in a device scalar (nvjpeg's counterpart: nvjpegEncodeRetrieveBitstreamDevice).  `encode` only enqueues work
on PyTorch's current stream -- no synchronisation, no copy -- so it can run inside a captured HIP graph (torch.cuda.graph,
sharding.FrameStreams.capture).  The bytes are those of `Jpeg.encode`.

    enc = DeviceJpeg()
    res = enc.encode(image, quality=94)   # returns at once
    data = res.to_host()                  # synchronises: a CPU uint8 tensor
    datas = retrieve([res1, res2, ...])   # one synchronisation for all lengths
"""

from __future__ import annotations

import torch

from ._native import lib
from ._streams import StreamBuffers
from .jpeg import InputFormat, JpegException, Subsampling
from .torch_darktable_extension import JpegInputFormat, JpegSubsampling, _ptr, _require, _stream


class DeviceJpegResult:
    """One encode: `data` is the stream's buffer (1-D uint8 on the device), `length` a 0-dim int64 on the device: the stream's
    length, or -1 when it did not fit in `data`.  Both are final once the stream the encode was issued on has got there."""

    def __init__(self, data: torch.Tensor, length: torch.Tensor, stream: torch.cuda.Stream):
        self.data, self.length, self.stream = data, length, stream

    def _wait(self) -> torch.cuda.Stream:
        here = torch.cuda.current_stream(self.data.device)
        here.wait_stream(self.stream)
        return here

    def to_host(self) -> torch.Tensor:
        """The stream as a CPU uint8 tensor (synchronises); JpegException if it did not fit in `data`."""
        with torch.cuda.device(self.data.device):
            self._wait()
            n = int(self.length.item())
            _check_length(n, self.data)
            return self.data[:n].cpu()


def _check_length(n: int, data: torch.Tensor) -> None:
    if n < 0:
        raise JpegException(f'nvjpegEncodeRetrieveBitstream, the stream does not fit in the output buffer ({data.numel()} bytes)')


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


class DeviceJpeg:
    """`Jpeg.encode` without a host round trip.  The coder's scratch is cached per (geometry, device, stream), so one object can
    serve several streams (one workspace each) and the calls of one stream reuse theirs."""

    def __init__(self):
        self._workspaces = StreamBuffers()

    @staticmethod
    def max_stream_bytes(width: int, height: int, subsampling=Subsampling.CSS_422, progressive: bool = False) -> int:
        """A capacity every stream of this geometry fits in (0 for an unsupported geometry)."""
        return int(lib.tdk_jpeg_device_max_stream_bytes(int(width), int(height), int(subsampling), int(bool(progressive))))

    def encode(self, image: torch.Tensor, quality: int = 94, input_format=InputFormat.RGBI, subsampling=Subsampling.CSS_422,
               progressive: bool = False, out: torch.Tensor | None = None) -> DeviceJpegResult:
        """Enqueue the encode of `image` (uint8 on the device, the layouts of Jpeg.encode) on the current stream.  `out`: a
        contiguous 1-D uint8 buffer on the image's device for the stream (default: a new one of max_stream_bytes)."""
        try:
            fmt, sub = JpegInputFormat(int(input_format)), JpegSubsampling(int(subsampling))
        except ValueError as e:
            raise RuntimeError(f'Invalid input format or subsampling: {e}') from e
        _require(image.is_cuda, 'Input image should be on CUDA device')
        _require(image.dtype == torch.uint8, 'Input image should be uint8')
        _require(image.is_contiguous(), 'Input data should be contiguous')
        if fmt in (JpegInputFormat.BGRI, JpegInputFormat.RGBI):
            _require(image.dim() == 3 and image.size(2) == 3, 'for interleaved (BGRI, RGBI) expected 3D tensor (H, W, C)')
            h, w = int(image.size(0)), int(image.size(1))
        else:
            _require(image.dim() == 3 and image.size(0) == 3, 'for planar (BGR, RGB) expected 3D tensor (C, H, W)')
            h, w = int(image.size(1)), int(image.size(2))
        if out is not None:
            _require(out.device == image.device, 'out must be on the device of the image')
            _require(out.dtype == torch.uint8, 'out must be uint8')
            _require(out.dim() == 1 and out.is_contiguous(), 'out must be a contiguous 1-D tensor')
        with torch.cuda.device(image.device):
            nbytes = lib.tdk_jpeg_device_workspace_bytes(w, h, int(sub))
            if nbytes == 0:
                raise JpegException(f'nvjpegEncodeImage, image {w}x{h} not supported')
            stream = torch.cuda.current_stream(image.device)
            ws = self._workspaces.get(nbytes, image.device, key=(w, h, int(sub), image.device))
            if out is None:
                out = torch.empty(self.max_stream_bytes(w, h, sub, progressive), dtype=torch.uint8, device=image.device)
            length = torch.empty((), dtype=torch.int64, device=image.device)
            rc = lib.tdk_jpeg_encode_device(_ptr(image), w, h, int(fmt), int(quality), int(sub), int(bool(progressive)), _ptr(ws), _ptr(out),
                                            out.numel(), _ptr(length), _stream())
            if rc != 0:
                raise JpegException(f'nvjpegEncodeImage, {lib.tdk_last_error().decode()}')
        return DeviceJpegResult(out, length, stream)

    def __repr__(self) -> str:
        return 'DeviceJpeg'


__all__ = ['DeviceJpeg', 'DeviceJpegResult', 'retrieve']
