"""One uint8 device buffer per CUDA stream, created on first use: the scratch an operator object keeps between its calls."""

from __future__ import annotations

import torch


class StreamBuffers:
    """An object that owns one may be used from several streams (or threads with different current streams) at once without its
    kernels sharing scratch: every stream gets a buffer of its own."""

    def __init__(self):
        self._buffers: dict[tuple, torch.Tensor] = {}

    def get(self, nbytes: int, device: torch.device, key=()) -> torch.Tensor:
        """The buffer of (key, the current stream of `device`), at least `nbytes` long: allocated when absent or smaller."""
        slot = (key, torch.cuda.current_stream(device).cuda_stream)
        buf = self._buffers.get(slot)
        if buf is None or buf.numel() < nbytes:
            buf = self._buffers[slot] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return buf

    def clear(self) -> None:
        self._buffers.clear()

    def __len__(self) -> int:
        return len(self._buffers)
