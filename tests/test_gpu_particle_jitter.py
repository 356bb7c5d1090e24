"""GPU tier: per-drop streak jitter on the device (rr_set_particle_jitter; k_particles<., true>, k_field_particles<false, ., true>,
k_rig_particles<false, ., true>).

  1. device records == the host statement (tools/particles.py expected_records(jitter=5)), bit for bit, counts included: i.i.d.,
     field (one chunk: store pass alone; three chunks: count pass + store pass) and rig (both stereo views with one and two
     chunks, then view 1 alone), each under counter and stream draws;
  2. set_particle_jitter(0) on the same context: today's records;
  3. the kernel profile: the launch counts with the jitter on are those with it off, and no k_noise_chains;
  4. every RR_E_ARG;  5. RainAugment(particle_model='field', draws='counter', jitter=5) == rr_pipeline_submit fed the host
     statement's records, and differs from the jitter = 0 batch."""
import importlib

import numpy as np
import pytest
import torch

import helpers as h
import particle_cases as cases
from test_gpu_augment import DEV, _planar, _scene, streaks_db          # noqa: F401  (streaks_db: a fixture)

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H

particles = importlib.import_module('rain-rendering_amd.tools.particles')
augment = importlib.import_module('rain-rendering_amd.augment')
imgops = importlib.import_module('rain-rendering_amd.common.imgops')
envmod = importlib.import_module('rain-rendering_amd.common.envmap')

JITTER = 5.0


def _check(rh, sims, want, what):
    got, cnt = rh.generate_drops(sims, H, W)
    for k in range(len(sims)):
        assert int(cnt[k]) == len(want[k]) > 100, (what, k)
        cases.same_nan_rotation(got[k], want[k], '%s: frame %d' % (what, k))
    return cnt


@pytest.mark.parametrize("draws", cases.DRAWS)
def test_iid_records_equal_host_statement(tmp_path, built, draws):
    sc = h.Scene(tmp_path, 64, 96, 10)                       # (only its streak database is used: the texture ratios)
    sims, dgrid, cdf, kw = cases.iid_run(cases.kitti())
    want = particles.expected_records(sims, dgrid, cdf, sc.db, draws=draws, jitter=JITTER, **kw)
    plain = particles.expected_records(sims, dgrid, cdf, sc.db, draws=draws, **kw)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        rh.set_particle_draws(draws)
        rh.set_particle_jitter(JITTER)
        cnt = _check(rh, sims, want, 'i.i.d., %s' % draws)
        # a capacity below the drop count: the count still tells, the records that fit are the first ones
        small, cnt_small = rh.generate_drops(sims, H, W, cap=max(len(want[0]) // 2, 1))
        assert np.array_equal(cnt_small, cnt)
        cases.same_nan_rotation(small[0], want[0][:len(want[0]) // 2], 'i.i.d., half the capacity')
        rh.set_particle_jitter(0)                            # back to today's records on the same context
        _check(rh, sims, plain, 'i.i.d., %s, jitter off again' % draws)
    finally:
        rh.close()
    assert want[0].tobytes() != plain[0].tobytes()


@pytest.mark.parametrize("draws", cases.DRAWS)
@pytest.mark.parametrize("chunks", [1, 3])
def test_field_records_equal_host_statement(tmp_path, built, chunks, draws):
    sc = h.Scene(tmp_path, 64, 96, 10)
    sims, dgrid, cdf, kw = cases.field_run(cases.kitti())
    want = particles.expected_records(sims, dgrid, cdf, sc.db, draws=draws, jitter=JITTER, **kw)
    plain = particles.expected_records(sims, dgrid, cdf, sc.db, draws=draws, **kw)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        rh.set_particle_model('field', kw['cam_hz'])
        rh.set_particle_draws(draws)
        rh.set_particle_jitter(JITTER)
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
        _check(rh, sims, want, 'field, %d chunks, %s' % (chunks, draws))
        rh.set_particle_jitter(0)
        _check(rh, sims, plain, 'field, %d chunks, %s, jitter off again' % (chunks, draws))
    finally:
        rh.close()
    assert want[1].tobytes() != plain[1].tobytes()


@pytest.mark.parametrize("draws", cases.DRAWS)
def test_rig_records_equal_host_statement(tmp_path, built, draws):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.kitti()
    hz = opt['cam_hz']
    sims1, dgrid, cdf = particles.sim_frames(opt, 25, 1, seed=1234 + 2 ** 40, model='rig', rig=cases.KITTI_STEREO)
    inst = [1, 2 ** 31 + 5]
    sims = particles.rig_run_sims(sims1, inst, 2)
    kw = dict(model='rig', cam_hz=hz, rig=cases.KITTI_STEREO)
    want = particles.expected_records(sims, dgrid, cdf, sc.db, draws=draws, jitter=JITTER, **kw)          # frame 2 i + v
    plain = particles.expected_records(sims, dgrid, cdf, sc.db, draws=draws, **kw)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        cases.set_rig(rh, opt)
        rh.set_particle_draws(draws)
        rh.set_particle_jitter(JITTER)
        for chunks in (1, 2):
            rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
            _check(rh, sims, want, 'rig, %d chunks, %s' % (chunks, draws))
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, 0)
        # view 1 alone: the same bits per view
        cases.set_rig(rh, opt, active=[1])
        got, _ = rh.generate_drops(particles.rig_run_sims(sims1, inst, 1), H, W)
        for i in range(len(inst)):
            cases.same_nan_rotation(got[i], want[2 * i + 1], 'active [1]: instant %d' % i)
        cases.set_rig(rh, opt)
        rh.set_particle_jitter(0)
        _check(rh, sims, plain, 'rig, %s, jitter off again' % draws)
    finally:
        rh.close()
    assert want[0].tobytes() != plain[0].tobytes()


def test_the_jitter_adds_no_launch(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.kitti()
    sims1, dgrid_r, cdf_r = particles.sim_frames(opt, 25, 1, seed=7, model='rig', rig=cases.KITTI_STEREO)
    rig_run = (particles.rig_run_sims(sims1, [1, 2], 2), dgrid_r, cdf_r, dict(model='rig', cam_hz=opt['cam_hz']))
    rh = cases.rain_hip(sc)
    try:
        rh.profile(True)
        for name, (sims, dgrid, cdf, kw) in (('k_particles', cases.iid_run(opt)), ('k_field_particles', cases.field_run(opt)), ('k_rig_particles', rig_run)):
            rh.set_particle_tables(dgrid, cdf)
            if kw['model'] == 'rig':
                cases.set_rig(rh, opt)
            else:
                rh.set_particle_model(kw['model'], kw.get('cam_hz', 0.0))
            for chunks in ((0,) if name == 'k_particles' else (1, 2)):
                rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
                for draws in cases.DRAWS:
                    rh.set_particle_draws(draws)
                    counts = {}
                    for deg in (0.0, JITTER):
                        rh.set_particle_jitter(deg)
                        rh.profile_reset()
                        rh.generate_drops(sims, H, W)
                        stats = rh.profile_read()
                        counts[deg] = {k: v[0] for k, v in stats.items()}
                        assert stats[name][0] >= 1 and 'k_noise_chains' not in stats, (name, draws, deg, stats)
                    assert counts[0.0] == counts[JITTER], (name, chunks, draws, counts)
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, 0)
    finally:
        rh.close()


def test_invalid_combinations_are_refused(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    sims, dgrid, cdf, _ = cases.iid_run(cases.kitti())
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        for bad in (-1.0, float('nan'), float('inf')):
            with pytest.raises(RuntimeError, match='jitter'):
                rh.set_particle_jitter(bad)
        # angular noise first, then the jitter (turning it off stays allowed)
        rh.set_particle_noise(2.0, 1.0, [0], [0])
        with pytest.raises(RuntimeError, match='jitter'):
            rh.set_particle_jitter(JITTER)
        rh.set_particle_jitter(0)
        rh.set_particle_noise(0.0, 0.0)
        # the jitter first, then angular noise (turning it off stays allowed); a record that names a run entry
        rh.set_particle_jitter(JITTER)
        with pytest.raises(RuntimeError, match='jitter'):
            rh.set_particle_noise(2.0, 1.0, [0], [0])
        rh.set_particle_noise(0.0, 0.0, [0], [0])
        bad = sims.copy()
        bad['run_pos'] = 1
        with pytest.raises(RuntimeError, match='jitter'):
            rh.generate_drops(bad, H, W)
        got, cnt = rh.generate_drops(sims, H, W)                # the context still works
        assert int(cnt[0]) > 100
    finally:
        rh.close()


def test_rain_augment_renders_the_host_statements_records(built, streaks_db):
    """RainAugment(particle_model='field', draws='counter', jitter=5), B = 2, bytes, KITTI, 25 mm/hr, against rr_pipeline_submit fed
    expected_records(jitter=5) as host tables: image bytes and mask equal; the jitter = 0 batch has other pixels."""
    kw = dict(streaks_db=streaks_db, sequence='data_object/training', particle_model='field', draws='counter')
    aug = augment.RainAugment('kitti', jitter=JITTER, **kw)
    plain_aug = None
    try:
        assert aug.frame_size() == (H, W)
        bgr, depth = _scene(2, H, W, seed=40)
        idx = [4, 5]
        p = aug.plan(25, idx)
        assert p['jitter'] == JITTER
        want = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, model='field', cam_hz=p['cam_hz'], draws='counter',
                                          jitter=JITTER)
        rainy, mask = aug(_planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV), 25, idx)
        rainy, mask = rainy.cpu().numpy(), mask.cpu().numpy()
        rh = h.hb.RainHip(0)
        try:
            rh.set_streak_db(aug.db.streaks_light)
            rh.set_camera(h.hb.make_camera(aug.focal, aug.f_number, aug.exposure))
            rh.set_prepass_kernels(imgops.gaussian_kernel(25, 25), imgops.gaussian_kernel(15, 0))
            we = rh.set_envmap_geometry(H, W, *envmod.EnvironmentMapGenerator(aug.focal, W, H).device_tables(H, W))
            rh.set_solid_angles(h.solid_angle.get_solid_angles(np.empty((H, we, 0))))
            frames = [dict(bg_u8=np.ascontiguousarray(bgr[i]), depth=np.ascontiguousarray(depth[i]), fog=tuple(p['fog'][i]), omega=None,
                           drops=want[i]) for i in range(2)]
            outs = [dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W))) for _ in range(2)]
            rh.pipeline_submit(0, frames, outs)
            while not rh.pipeline_wait(0):
                rh.pipeline_submit(0, frames, outs)
        finally:
            rh.close()
        for i in range(2):
            assert len(want[i]) > 100
            assert np.array_equal(rainy[i].transpose(1, 2, 0), outs[i]['image_u8']), i
            assert np.array_equal(mask[i, 0], outs[i]['mask'].astype(np.float32)), i
            assert outs[i]['mask'].max() > 0, i
        plain_aug = augment.RainAugment('kitti', **kw)
        rainy_0, _ = plain_aug(_planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV), 25, idx)
        assert not np.array_equal(rainy_0.cpu().numpy(), rainy)
    finally:
        aug.close()
        if plain_aug is not None:
            plain_aug.close()
