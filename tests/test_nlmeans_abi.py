"""CPU-only: the third header include/tdk_hip_denoise.h (non-local means) -- it parses to exactly its three declarations
(exports and the ctypes table: tests/test_header_abi.py), every argument error of tdk_nlmeans is reported on
the host before any HIP call, and the Python front-end torch_darktable.NLMeans raises the error types of Wiener."""

import ctypes
import re
from pathlib import Path

import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_denoise.h'
EXPECTED = ['tdk_denoise_abi_version', 'tdk_nlmeans', 'tdk_nlmeans_lds_bytes']


def test_header_declares_the_denoise_surface(td):
    from torch_darktable import _native

    assert sorted(declarations(HEADER)) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_DENOISE_ABI_VERSION 1\b', text)
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert _native.ABI_VERSIONS['tdk_denoise_abi_version'] == (1, 'denoise ABI')


def test_nlmeans_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches memory or a device
    names = ['image', 'out', 'w', 'h', 'c', 'dtype', 'S', 'P', 'strength', 'cw', 'stream']
    args = [fake, fake + (1 << 24), 64, 48, 3, 0, 7, 2, 0.1, None, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_nlmeans(*a)

    def weights(*v):
        return ctypes.cast((ctypes.c_float * len(v))(*v), ctypes.c_void_p)

    for k in ('image', 'out'):
        assert call(**{k: None}) == 1 and b'null pointer' in lib.tdk_last_error(), k
    for k in ('w', 'h'):
        for v in (0, -3):
            assert call(**{k: v}) == 1 and b'outside' in lib.tdk_last_error(), (k, v)
    for c in (0, 2, 4):
        assert call(c=c) == 1 and b'channels' in lib.tdk_last_error(), c
    assert call(dtype=2) == 1 and b'dtype' in lib.tdk_last_error()
    for s in (0, 11, -1):
        assert call(S=s) == 1 and b'search_radius' in lib.tdk_last_error(), s
    for p in (0, 5, -1):
        assert call(P=p) == 1 and b'patch_radius' in lib.tdk_last_error(), p
    for strength in (0.0, -0.1, float('inf'), float('nan')):
        assert call(strength=strength) == 1 and b'h must be' in lib.tdk_last_error(), strength
    assert call(cw=weights(1.0, -0.5, 1.0)) == 1 and b'channel weight' in lib.tdk_last_error()
    assert call(cw=weights(1.0, float('nan'), 1.0)) == 1 and b'channel weight' in lib.tdk_last_error()
    assert call(cw=weights(0.0, 0.0, 0.0)) == 1 and b'all zero' in lib.tdk_last_error()
    assert call(c=1, cw=weights(0.0)) == 1 and b'all zero' in lib.tdk_last_error()
    assert call(out=fake) == 1 and b'overlap' in lib.tdk_last_error()
    assert call(out=fake + 64) == 1 and b'overlap' in lib.tdk_last_error()


def test_nlmeans_lds_query_runs_on_the_host(td):
    from torch_darktable._native import lib

    for bad in ((0, 2, 3), (11, 2, 3), (7, 0, 3), (7, 5, 3), (7, 2, 2), (7, 2, 0)):
        assert lib.tdk_nlmeans_lds_bytes(*bad) == 0, bad
    assert 0 < lib.tdk_nlmeans_lds_bytes(1, 1, 1) < lib.tdk_nlmeans_lds_bytes(7, 2, 1) < lib.tdk_nlmeans_lds_bytes(7, 2, 3) < lib.tdk_nlmeans_lds_bytes(10, 4, 3)


def test_package_exports_nlmeans(td):
    import torch_darktable

    assert torch_darktable.NLMeans is torch_darktable.nlmeans.NLMeans
    assert 'NLMeans' in torch_darktable.__all__ and 'nlmeans' in torch_darktable.__all__
    assert torch_darktable.nlmeans.__all__ == ['NLMeans']
    for method in ('process', 'process_luminance', 'process_log_luminance'):
        assert callable(getattr(torch_darktable.NLMeans, method))


def test_python_front_end_raises_the_error_types_of_wiener(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: nothing below reaches the GPU
    with pytest.raises(ValueError, match='CUDA'):
        td.NLMeans(torch.device('cpu'), (64, 48))
    for size in ((0, 48), (64, -1)):
        with pytest.raises(ValueError, match='positive'):
            td.NLMeans(cuda, size)
    for s in (0, 11):
        with pytest.raises(ValueError, match='search_radius'):
            td.NLMeans(cuda, (64, 48), search_radius=s)
    for p in (0, 5):
        with pytest.raises(ValueError, match='patch_radius'):
            td.NLMeans(cuda, (64, 48), patch_radius=p)
    nlm = td.NLMeans(cuda, (64, 48))
    assert (nlm.search_radius, nlm.patch_radius) == (7, 2) and 'NLMeans(64x48' in repr(nlm)
    with pytest.raises(RuntimeError, match='shape'):
        nlm.process(torch.zeros(48, 60, 3), 0.1)
    with pytest.raises(RuntimeError, match='shape'):
        nlm.process(torch.zeros(64, 48, 3), 0.1)
    with pytest.raises(ValueError, match='channels'):
        nlm.process(torch.zeros(48, 64, 2), 0.1)
    for h in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='h must be'):
            nlm.process(torch.zeros(48, 64, 3), h)
    with pytest.raises(ValueError, match='3 elements'):
        nlm.process(torch.zeros(48, 64, 3), 0.1, [1.0])
    for cw in ([1.0, -1.0, 1.0], [0.0, 0.0, 0.0], [1.0, float('nan'), 1.0]):
        with pytest.raises(ValueError, match='channel_weights'):
            nlm.process(torch.zeros(48, 64, 3), 0.1, cw)
    with pytest.raises(RuntimeError, match='CUDA'):
        nlm.process(torch.zeros(48, 64, 3), 0.1)   # no CPU fallback
