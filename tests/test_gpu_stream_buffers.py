"""GPU: torch_darktable._streams.StreamBuffers, the per-stream scratch of the operator objects -- one buffer per (key, stream), grown
for that stream alone, dropped by clear().  Allocations only: no kernel is launched."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_one_buffer_per_key_and_stream(td):
    from torch_darktable._streams import StreamBuffers

    dev = torch.device('cuda', 0)
    buffers = StreamBuffers()
    assert len(buffers) == 0
    main = buffers.get(1024, dev)
    assert main.dtype == torch.uint8 and main.device == dev and main.numel() == 1024
    assert buffers.get(1024, dev) is main and buffers.get(512, dev) is main   # the same stream: the same tensor, a smaller request too
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    side = []
    for s in (s1, s2, s1, s2):
        with torch.cuda.stream(s):
            side.append(buffers.get(1024, dev))
    assert side[0] is side[2] and side[1] is side[3]
    assert side[0] is not side[1] and side[0] is not main and side[1] is not main
    assert len({t.data_ptr() for t in (main, side[0], side[1])}) == 3 and len(buffers) == 3

    with torch.cuda.stream(s1):   # a larger request replaces the buffer of that stream alone
        grown = buffers.get(2048, dev)
        assert grown is not side[0] and grown.numel() == 2048 and buffers.get(1024, dev) is grown
    with torch.cuda.stream(s2):
        assert buffers.get(1024, dev) is side[1]
    assert buffers.get(1024, dev) is main and len(buffers) == 3

    a, b = buffers.get(1024, dev, key=(64, 48)), buffers.get(1024, dev, key=(48, 64))   # distinct keys on one stream
    assert a is not b and a is not main and b is not main and len(buffers) == 5
    assert buffers.get(1024, dev, key=(64, 48)) is a and buffers.get(1024, dev) is main

    buffers.clear()
    assert len(buffers) == 0
    assert buffers.get(1024, dev) is not main and len(buffers) == 1
