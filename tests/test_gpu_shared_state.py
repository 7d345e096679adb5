"""GPU: the per-(device, stream) cached state of compute_image_bounds (the ticket state) and compute_image_metrics (the
MetricsAccumulator) when host threads share a stream -- the default stream is everyone's.

The interleaving is made deterministic, not provoked by a stress loop: a stand-in for the native library forwards every call
and, right after thread A's first launch, lets thread B run a whole call on the same stream before A goes on.  B's call may
only start when A's list is complete (the state's lock), so the stand-in waits for B with a short timeout: with the lock it
times out and A finishes first, without it B's list lands between A's launches.  Both threads' results must be right either way.
A list cut short by KeyboardInterrupt must not leave tickets or half-accumulated sums for the next call on that stream."""

import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LAUNCHES = ('tdk_image_bounds', 'tdk_image_metrics_accumulate_rows', 'tdk_image_metrics')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


class _Library:
    """The native library with a hook in front of the launches of the cached-state paths: hook(name) runs before each."""

    def __init__(self, real, hook):
        self._real, self._hook = real, hook

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in LAUNCHES:
            return fn

        def launch(*args):
            return self._hook(name, lambda: fn(*args))

        return launch


def _images(dev, shapes, offset, scale, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return [(torch.rand(h, w, 3, generator=g) * scale + offset).to(dev) for h, w in shapes]


def _bounds_ref(images, stride):
    s = [i.cpu().numpy().astype(np.float64)[::stride, ::stride] for i in images]
    return np.array([min(x.min() for x in s), max(x.max() for x in s)], np.float32)


def _interleave(monkeypatch, ext, call_a, call_b):
    """Run call_a() on this thread; B runs call_b() as a whole right after A's first launch (or as soon as the lock lets it)."""
    a_ident = threading.get_ident()
    a_launched, b_done = threading.Event(), threading.Event()
    first = [True]

    def hook(name, launch):
        r = launch()
        if threading.get_ident() == a_ident and first[0]:
            first[0] = False
            a_launched.set()
            b_done.wait(1.0)  # a correct lock keeps B out until A's list is done: time out instead of deadlocking
        return r

    monkeypatch.setattr(ext, 'lib', _Library(ext.lib, hook))
    box = {}

    def thread_b():
        try:
            assert a_launched.wait(30.0), 'thread A never launched'
            box['b'] = call_b()
        except BaseException as e:  # noqa: BLE001  (re-raised on the main thread)
            box['error'] = e
        finally:
            b_done.set()

    tb = threading.Thread(target=thread_b)
    tb.start()
    try:
        a = call_a()
    finally:
        tb.join(60.0)
    assert not tb.is_alive(), 'thread B did not finish'
    if 'error' in box:
        raise box['error']
    assert not first[0], 'the hook never ran: the launch names changed'
    torch.cuda.synchronize()
    return a, box['b']


def test_bounds_lists_of_two_threads_on_one_stream(td, dev, monkeypatch):
    from torch_darktable import torch_darktable_extension as ext

    a_imgs = _images(dev, [(96, 128), (200, 300)], 0.0, 1.0, 1)      # values in [0, 1)
    b_imgs = _images(dev, [(64, 64), (150, 90)], 10.0, 5.0, 2)       # values in [10, 15): any mixing shows
    a, b = _interleave(monkeypatch, ext, lambda: td.compute_image_bounds(a_imgs, 8), lambda: td.compute_image_bounds(b_imgs, 8))
    assert np.array_equal(a.cpu().numpy(), _bounds_ref(a_imgs, 8)), (a, _bounds_ref(a_imgs, 8))
    assert np.array_equal(b.cpu().numpy(), _bounds_ref(b_imgs, 8)), (b, _bounds_ref(b_imgs, 8))
    monkeypatch.undo()
    assert np.array_equal(td.compute_image_bounds(a_imgs, 4).cpu().numpy(), _bounds_ref(a_imgs, 4))  # the state came back idle


def test_metrics_lists_of_two_threads_on_one_stream(td, oracle, dev, monkeypatch):
    from torch_darktable import torch_darktable_extension as ext

    a_imgs = _images(dev, [(96, 128), (200, 300)], 0.0, 1.0, 3)
    b_imgs = _images(dev, [(64, 64), (150, 90)], 0.2, 0.5, 4)
    a, b = _interleave(monkeypatch, ext, lambda: td.compute_image_metrics(a_imgs, stride=8), lambda: td.compute_image_metrics(b_imgs, stride=2))
    ref_a = oracle.image_metrics([i.cpu().numpy() for i in a_imgs], 8)
    ref_b = oracle.image_metrics([i.cpu().numpy() for i in b_imgs], 2)
    assert np.allclose(a.cpu().numpy(), ref_a, rtol=2e-5, atol=2e-6), (a, ref_a)
    assert np.allclose(b.cpu().numpy(), ref_b, rtol=2e-5, atol=2e-6), (b, ref_b)


def test_keyboard_interrupt_in_a_list_leaves_the_state_clean(td, oracle, dev, monkeypatch):
    from torch_darktable import torch_darktable_extension as ext

    imgs = _images(dev, [(96, 128), (200, 300)], -0.5, 3.0, 5)
    calls = {}

    def hook(name, launch):  # the second launch of the list never happens
        n = calls[name] = calls.get(name, 0) + 1
        if (name == 'tdk_image_bounds' and n == 2) or name == 'tdk_image_metrics':
            raise KeyboardInterrupt
        return launch()

    monkeypatch.setattr(ext, 'lib', _Library(ext.lib, hook))
    with pytest.raises(KeyboardInterrupt):
        td.compute_image_bounds(imgs, 8)
    with pytest.raises(KeyboardInterrupt):
        td.compute_image_metrics(imgs, stride=4)
    assert calls == {'tdk_image_bounds': 2, 'tdk_image_metrics_accumulate_rows': 1, 'tdk_image_metrics': 1}
    monkeypatch.undo()
    nxt = _images(dev, [(128, 160)], 0.1, 0.8, 6)
    got_b = td.compute_image_bounds(nxt, 8).cpu().numpy()
    got_m = td.compute_image_metrics(nxt, stride=4).cpu().numpy()
    assert np.array_equal(got_b, _bounds_ref(nxt, 8)), (got_b, _bounds_ref(nxt, 8))
    ref_m = oracle.image_metrics([nxt[0].cpu().numpy()], 4)
    assert np.allclose(got_m, ref_m, rtol=2e-5, atol=2e-6), (got_m, ref_m)
