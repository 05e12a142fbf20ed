"""The argument checkers of native.py, one per kind of argument: they read shapes, strides and addresses only, so host
tensors serve and neither a device nor the shared object is needed."""
import types

import numpy as np
import pytest
import torch

from image_stitcher_amd import native


def _t():
    return torch.zeros((3, 8, 8), dtype=torch.uint16)


def _b():
    return torch.zeros((2, 4, 8, 8), dtype=torch.uint8)


@pytest.mark.parametrize('make,want', [
    (lambda: _t(), (3, 8, 8, 64, 8)),
    (lambda: _t()[::2], (2, 8, 8, 128, 8)),
    (lambda: torch.zeros((3, 8, 12))[:, :, :8], (3, 8, 8, 96, 12)),
    (lambda: _b(), (8, 8, 8, 64, 8)),
    (lambda: _b()[:, ::2], (4, 8, 8, 128, 8)),
    (lambda: torch.zeros((1, 1, 5))[0], (1, 1, 5, 5, 5)),
    (lambda: torch.zeros((8, 8)), (1, 8, 8, 64, 8)),
])
def test_plane_layout(make, want):
    assert native._plane_layout(make(), 'x') == want


@pytest.mark.parametrize('make', [
    lambda: _t().permute(0, 2, 1),
    lambda: _t()[:1].expand(3, 8, 8),
    lambda: _b()[:, :3],
    lambda: _t()[:, :, :0],
    lambda: torch.zeros((3, 8, 16))[:, :, ::2],
])
def test_plane_layout_refuses(make):
    with pytest.raises(ValueError):
        native._plane_layout(make(), 'x')


def test_byte_extents():
    t = _t()
    extent = lambda v: native._byte_extent(v, native._plane_layout(v, 'x'))
    assert extent(t) == (t.data_ptr(), t.data_ptr() + 3 * 64 * 2)
    assert extent(t[::2]) == (t.data_ptr(), t.data_ptr() + (128 + 64) * 2)
    assert native._overlap(extent(t[:2]), extent(t[1:]))
    assert not native._overlap(extent(t[:1]), extent(t[2:]))
    assert native._overlap(extent(t[::2]), extent(t[1::2]))      # interleaved views share no element, their ranges do


def test_projected_planes():
    plan = lambda n: types.SimpleNamespace(n_tiles=n)
    assert native._projected_planes(plan(4), torch.zeros((3, 4, 8, 8)), None, None) == 3
    assert native._projected_planes(plan(4), torch.zeros((4, 8, 8)), None, None) == 1
    assert native._projected_planes(plan(4), None, torch.zeros(12, dtype=torch.int64), None) == 3
    assert native._projected_planes(plan(0), None, torch.zeros(0, dtype=torch.int64), [None, None]) == 2
    with pytest.raises(ValueError):
        native._projected_planes(plan(4), None, None, None)


def test_z_level_words():
    words = native._z_level_words([0, 2 ** 32 - 1], False)
    assert words.dtype == np.int32 and words.tolist() == [0, -1]
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match='z levels'):
            native._z_level_words([0, bad], False)
    assert native._z_level_words([5, 5], False).tolist() == [5, 5]
    with pytest.raises(ValueError, match='distinct'):
        native._z_level_words([5, 5], True)


def test_int_in():
    lo, hi = 1, 127
    for bad in (True, 3.0, lo - 1, hi + 1):
        with pytest.raises(ValueError, match='radius'):
            native._int_in(bad, lo, hi, 'radius')
    assert native._int_in(np.int64(lo), lo, hi, 'radius') == lo
    assert native._int_in(hi, lo, hi, 'radius') == hi


def test_device_checks_sit_in_the_helpers():
    for integer_only in (False, True):
        with pytest.raises(ValueError):
            native._plane_stack(_t(), 'planes', integer_only)
    with pytest.raises(ValueError):
        native._check_plane('out', torch.zeros((8, 8)), (8, 8))
