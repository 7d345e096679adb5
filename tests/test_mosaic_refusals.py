"""CPU-only: every row of tests/mosaic_refusals.py -- what the stages on raw mosaics refuse, with which exception and in which words,
which of two wrong arguments they name, and how they print.  No row needs a GPU: objects are built for cuda:0 and never run."""

import re

import pytest
import torch

import mosaic_refusals as table
from mosaic_refusals import New


@pytest.fixture(autouse=True)
def no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)   # (what the constructors ask: nothing is allocated on any machine)


def resolve(td, value):
    """A value of the table with every `New` in it built."""
    if isinstance(value, New):
        return build(td, value.cls, value.kwargs)
    if isinstance(value, (list, tuple)):
        return type(value)(resolve(td, v) for v in value)
    return value


def build(td, cls: str, kwargs: dict):
    from torch_darktable.pipeline import image_processor

    target = image_processor if cls == 'ImageProcessor' else td
    for part in cls.split('.'):
        target = getattr(target, part)
    if not callable(target):   # a member of an enumeration
        return target
    merged = {**table.BASE.get(cls, {}), **kwargs}
    return target(**{name: resolve(td, value) for name, value in merged.items()})


def refused(exception, message, call):
    with pytest.raises(exception) as caught:
        call()
    assert type(caught.value) is exception, type(caught.value)
    assert re.search('^' + re.escape(message) + '$', str(caught.value.args[0])), caught.value.args[0]


def test_the_table_is_whole():
    assert table.ROWS == len(table.CONSTRUCT) + len(table.REPRS) + len(table.CALLS) >= 500
    stages = {'RawPrepare', 'Highlights', 'ChromaticAberration', 'NoiseProfile', 'TemporalDenoise', 'MotionEstimate', 'MotionTemporalDenoise', 'HdrMerge',
              'MotionHdrMerge', 'FrameStats'}
    assert stages <= {row[0] for row in table.CONSTRUCT} and stages == {row[0] for row in table.REPRS} and stages <= {row[0] for row in table.CALLS}
    for stage in stages:
        assert sum(1 for row in table.REPRS if row[0] == stage) >= 2, stage


@pytest.mark.parametrize('row', range(len(table.CONSTRUCT)), ids=lambda i: f'{i}-{table.CONSTRUCT[i][0]}')
def test_constructor_refusals(td, row):
    cls, kwargs, exception, message = table.CONSTRUCT[row]
    refused(exception, message, lambda: build(td, cls, kwargs))


@pytest.mark.parametrize('row', range(len(table.REPRS)), ids=lambda i: f'{i}-{table.REPRS[i][0]}')
def test_reprs(td, row):
    cls, kwargs, text = table.REPRS[row]
    stage = build(td, cls, kwargs)
    assert repr(stage) == text
    assert stage.image_size == (stage.width, stage.height) == tuple(kwargs.get('image_size', table.SIZE))


@pytest.mark.parametrize('row', range(len(table.CALLS)), ids=lambda i: f'{i}-{table.CALLS[i][0]}.{table.CALLS[i][2]}')
def test_call_refusals(td, row):
    cls, kwargs, method, args, call_kwargs, exception, message = table.CALLS[row]
    stage = build(td, cls, kwargs)
    refused(exception, message, lambda: getattr(stage, method)(*resolve(td, args), **{name: resolve(td, value) for name, value in call_kwargs.items()}))
