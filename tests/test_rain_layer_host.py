"""CPU tier of the rain layer: the reference maker of tests/rain_layer.py on trial before the GPU tier uses it -- its
own condition (nothing clamps, the composite is affine in the image, one transmittance for the three channels) on an oracle
catalogue, a frame smaller than one tile and the 8232-record table of the host build -- and the layout of the new C structs."""
import ctypes
import importlib

import numpy as np
import pytest

import compositor_cases as cc
import helpers as h
import rain_layer as rl


@pytest.fixture(scope='module')
def tpl(tmp_path_factory):
    return cc.Templates(tmp_path_factory.mktemp('tpl'))


def _case(name, tpl, tmp_path_factory):
    if name == 'seams_low':
        return cc.seams(tmp_path_factory.mktemp('sl'), tpl, 'low')
    if name == 'segment_dim':
        return rl.segment_dim(tmp_path_factory.mktemp('sd'), tpl)
    return next(c for c in cc.shapes(lambda n: tmp_path_factory.mktemp(n), tpl) if c.name == name)


@pytest.mark.parametrize('name', ['seams_low', 'tiles_3', 'segment_dim'])
def test_reference_condition(name, tpl, tmp_path_factory):
    """reference() asserts its condition itself; here it must also describe a frame with rain on it."""
    c = _case(name, tpl, tmp_path_factory)
    ref = rl.reference(c)
    print('%s: peak %.3f, affine error %.3g, max n %d, max L %.3f, min T %.3f' % (name, ref['peak'], ref['affine'], ref['n'].max(), ref['L'].max(),
                                                                                 ref['T'].min()))
    assert ref['L'].shape == (c.H, c.W, 3) and ref['T'].shape == ref['n'].shape == (c.H, c.W)
    assert ref['n'].max() > 0 and ref['L'].max() > 0 and ref['T'].min() < 1
    rained = (ref['T'] != 1) | (ref['L'] != 0).any(axis=2)
    assert not (rained & (ref['n'] == 0)).any(), 'rain outside every listed box'
    assert ((ref['T'] == 1) & (ref['L'] == 0).all(axis=2))[ref['n'] == 0].all()
    assert (ref['T'] >= 0).all() and (ref['T'] <= 1).all() and (ref['L'] >= 0).all()
    assert (rl.bound(ref)[ref['n'] == 0] == 1e-9).all() and rl.bound(ref).max() == ref['n'].max() * 2.0 ** -21 + 1e-9


def test_segment_itself_saturates(tpl, tmp_path_factory):
    """Why the GPU tier renders the 8232 records under a dimmer map: cc.segment's own frame does not meet the condition."""
    c = cc.segment(tmp_path_factory.mktemp('sg'), tpl)
    c.name = 'segment_dim'                       # (the host build, as for the dim case)
    with pytest.raises(AssertionError):
        rl.reference(c)


def test_struct_sizes(built):
    lib = h.hb.load_library()
    assert lib.rr_sizeof_layer_out() == ctypes.sizeof(h.hb.rr_layer_out) == 16
    assert lib.rr_sizeof_pipeline_layer() == ctypes.sizeof(h.hb.rr_pipeline_layer) == 16
    assert lib.rr_sizeof_tensor_layer() == ctypes.sizeof(h.hb.rr_tensor_layer) == 24
    for name in ('rr_pipeline_set_layer', 'rr_augment_set_layer'):
        assert name in h.hb.EXPORTS and hasattr(lib, name)


def test_existing_abi_is_unchanged(built):
    lib = h.hb.load_library()
    assert lib.rr_version() == 400
    assert lib.rr_sizeof_frame_out() == 72 and lib.rr_sizeof_tensor_batch() == 72


def test_want_layer_and_return_layer_take_bools_only(built):
    """Validation before any device work (no context is needed to refuse)."""
    rh = object.__new__(h.hb.RainHip)
    with pytest.raises(ValueError):
        with rh._layer_armed([], 1):
            pass
    aug = importlib.import_module('rain-rendering_amd.augment')
    with pytest.raises(ValueError):
        aug.RainAugment(return_layer=1)
