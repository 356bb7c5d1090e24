"""CPU tier of RainAugment (rain-rendering_amd/augment.py): what a call sends -- rr_sim_frame records, diameter tables, fog
constants -- against what the `main.py --device_particles` driver builds, and the input checks, all without a GPU."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import helpers as h

augment = importlib.import_module('rain-rendering_amd.augment')
particles = importlib.import_module('rain-rendering_amd.tools.particles')
dbmod = importlib.import_module('rain-rendering_amd.common.db')
fogmod = importlib.import_module('rain-rendering_amd.common.add_attenuation')

SEQ = 'data_object/training'


@pytest.fixture(scope='module')
def aug(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('augdb'))
    h.synthetic.write_streak_db(os.path.join(root, 'rainstreakdb'))
    return augment.RainAugment('kitti', streaks_db=os.path.join(root, 'rainstreakdb'), sequence=SEQ)


def _driver(rate, n_frames=None):
    """The driver's set-up of one (sequence, intensity) run (common/generator.py, --device_particles)."""
    st = dbmod.settings('kitti')
    opts = dbmod.sim('kitti', SEQ, os.path.join('particles', 'kitti'))['options']
    n_sim = particles.n_sim_frames(opts)
    sims, dgrid, cdf = particles.sim_frames(opts, rate, n_sim, render_scale=st['render_scale'], seed=0)
    fog = fogmod.FogRain(rain_intensity=rate, focal=st['cam_focal'] / 1000., f_number=st['cam_f_number'], angle=90,
                         exposure=st['cam_exposure'], camera_gain=st['cam_gain']).constants()
    return n_sim, sims, dgrid, np.atleast_2d(cdf), fog


def test_records_tables_and_fog_are_the_drivers(aug):
    n_sim, sims, dgrid, cdf, fog = _driver(25)
    idx = [0, 1, 7, n_sim - 1, n_sim, 3 * n_sim + 5]
    p = aug.plan(25, idx)
    assert aug.n_sim == n_sim
    assert np.array_equal(p['d_grid'], dgrid) and np.array_equal(p['cdf'], cdf)
    for i, f in enumerate(idx):
        want = sims[f % n_sim].copy()
        want['draw_seed'] = f
        assert p['sims'][i].tobytes() == want.tobytes(), (i, f)
        assert tuple(p['fog'][i]) == tuple(fog)
    assert p['drops_cap'] == (min(max(1024, int(sims['n_particles'].max())), 2 ** 16) + 3) // 4 * 4


def test_mixed_intensities_index_the_right_tables(aug):
    rates, idx = [5, 25, 100, 25, 5], [3, 4, 5, 6, 200]
    p = aug.plan(rates, idx)
    assert p['key'] == (5.0, 25.0, 100.0)
    for i, (r, f) in enumerate(zip(rates, idx)):
        n_sim, sims, dgrid, cdf, fog = _driver(r)
        want = sims[f % n_sim].copy()
        want['draw_seed'] = f
        got = p['sims'][i].copy()
        assert np.array_equal(p['cdf'][int(got['table'])], cdf[int(want['table'])]), (r, f)
        got['table'] = want['table']
        assert got.tobytes() == want.tobytes(), (r, f)
        assert tuple(p['fog'][i]) == tuple(fog)
    # one union per set of intensities, whatever their order
    assert aug.plan([100, 5, 25], [0, 0, 0])['cdf'] is p['cdf']
    assert len(p['cdf']) == sum(len(_driver(r)[3]) for r in (5, 25, 100))


def _inputs(B=1, H=375, W=1242, dtype=torch.uint8):
    return torch.zeros((B, 3, H, W), dtype=dtype), torch.ones((B, H, W), dtype=torch.float32)


def test_every_input_check_raises_before_any_gpu_call(aug):
    img, dep = _inputs()
    with pytest.raises(ValueError, match='GPU'):                     # a CPU tensor
        aug(img, dep, 25, [0])
    with pytest.raises(ValueError, match='GPU'):
        aug(img.to('meta'), dep, 25, [0])
    with pytest.raises(TypeError, match='uint8 or float32'):
        aug(img.to(torch.int16), dep, 25, [0])
    with pytest.raises(TypeError, match='uint8 or float32'):
        aug(img.to(torch.float64), dep, 25, [0])
    with pytest.raises(ValueError, match=r'\[B, 3, H, W\]'):
        aug(img[0], dep, 25, [0])
    with pytest.raises(ValueError, match=r'\[B, 3, H, W\]'):
        aug(torch.zeros((1, 4, 375, 1242), dtype=torch.uint8), dep, 25, [0])
    with pytest.raises(ValueError, match='depth'):
        aug(img, dep.to(torch.float64), 25, [0])
    with pytest.raises(ValueError, match='depth'):
        aug(img, dep[:, :-1], 25, [0])
    with pytest.raises(ValueError, match='depth'):
        aug(img, dep[:, None].expand(1, 2, 375, 1242), 25, [0])
    with pytest.raises(ValueError, match='intensity'):
        aug(img, dep, 0, [0])
    with pytest.raises(ValueError, match='intensity'):
        aug(img, dep, [-5], [0])
    with pytest.raises(ValueError, match='frame_index'):
        aug(img, dep, 25, [-1])
    with pytest.raises(ValueError, match='frame_index'):
        aug(img, dep, 25, [0, 1])                                      # one index per image
    with pytest.raises(ValueError, match='375 x 1242'):                # not the size this dataset's simulation renders
        aug(*_inputs(H=96, W=160), 25, [0])
    # [B, 1, H, W] depth is accepted: the check that fails is the device
    with pytest.raises(ValueError, match='GPU'):
        aug(img, dep[:, None], 25, 0)


def test_tensor_batch_struct_size(built):
    hb = importlib.import_module('rain-rendering_amd.hip_backend')
    lib = hb.load_library()
    assert lib.rr_sizeof_tensor_batch() == ctypes.sizeof(hb.rr_tensor_batch) == 72
