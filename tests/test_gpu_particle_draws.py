"""GPU tier: counter-based per-drop draws on the device (rr_set_particle_draws RR_DRAWS_COUNTER; k_particles<true>,
k_field_particles<., true>, k_rig_particles<., true>).

  1. device records == the host statement (tools/particles.py expected_records(draws='counter')), bit for bit, counts included:
     i.i.d., field (one chunk: store pass alone; three chunks: count pass + store pass) and rig (both stereo views, then view 1 alone);
  2. a capacity below the drop count; 3. back to RR_DRAWS_STREAM on the same context: today's records;
  4. the kernel profile: no k_particle_draws launch in counter mode; 5. every RR_E_ARG;
  6. RainAugment(draws='counter') == rr_pipeline_submit fed the host statement's records."""
import importlib

import numpy as np
import pytest
import torch

import helpers as h
import particle_cases as cases
from test_gpu_augment import DEV, _planar, _scene, streaks_db          # noqa: F401  (streaks_db: a fixture)

pytestmark = pytest.mark.gpu

particles = importlib.import_module('rain-rendering_amd.tools.particles')
augment = importlib.import_module('rain-rendering_amd.augment')
imgops = importlib.import_module('rain-rendering_amd.common.imgops')
envmod = importlib.import_module('rain-rendering_amd.common.envmap')

W, H = cases.W, cases.H


def _check(rh, sims, want, what):
    got, cnt = rh.generate_drops(sims, H, W)
    for k in range(len(sims)):
        assert int(cnt[k]) == len(want[k]) > 100, (what, k)
        cases.same_bytes(got[k], want[k], '%s: frame %d' % (what, k))
    return cnt


def test_iid_records_equal_host_statement(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)                       # (only its streak database is used: the texture ratios)
    sims, dgrid, cdf, kw = cases.iid_run(cases.kitti())
    want = particles.expected_records(sims, dgrid, cdf, sc.db, draws='counter', **kw)
    stream = particles.expected_records(sims, dgrid, cdf, sc.db, **kw)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        rh.set_particle_draws('counter')
        cnt = _check(rh, sims, want, 'i.i.d.')
        # a capacity below the drop count: the count still tells, the records that fit are the first ones
        small, cnt_small = rh.generate_drops(sims, H, W, cap=max(len(want[0]) // 2, 1))
        assert np.array_equal(cnt_small, cnt)
        assert len(small[0]) == len(want[0]) // 2 and small[0].tobytes() == want[0][:len(small[0])].tobytes()
        # back to the stream on the same context: today's records
        rh.set_particle_draws('stream')
        _check(rh, sims, stream, 'i.i.d., stream again')
    finally:
        rh.close()
    assert want[0].tobytes() != stream[0].tobytes()


@pytest.mark.parametrize("chunks", [1, 3])
def test_field_records_equal_host_statement(tmp_path, built, chunks):
    sc = h.Scene(tmp_path, 64, 96, 10)
    sims, dgrid, cdf, kw = cases.field_run(cases.kitti())
    want = particles.expected_records(sims, dgrid, cdf, sc.db, draws='counter', **kw)
    stream = particles.expected_records(sims, dgrid, cdf, sc.db, **kw)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        rh.set_particle_model('field', kw['cam_hz'])
        rh.set_particle_draws('counter')
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
        cnt = _check(rh, sims, want, 'field, %d chunks' % chunks)
        small, cnt_small = rh.generate_drops(sims, H, W, cap=max(len(want[1]) // 2, 1))
        assert np.array_equal(cnt_small, cnt)
        assert len(small[1]) == len(want[1]) // 2 and small[1].tobytes() == want[1][:len(small[1])].tobytes()
        rh.set_particle_draws('stream')
        _check(rh, sims, stream, 'field, %d chunks, stream again' % chunks)
    finally:
        rh.close()


def test_rig_records_equal_host_statement(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.kitti()
    hz = opt['cam_hz']
    sims1, dgrid, cdf = particles.sim_frames(opt, 25, 1, seed=1234 + 2 ** 40, model='rig', rig=cases.KITTI_STEREO)
    inst = [1, 2 ** 31 + 5]
    sims = particles.rig_run_sims(sims1, inst, 2)
    kw = dict(model='rig', cam_hz=hz, rig=cases.KITTI_STEREO)
    want = particles.expected_records(sims, dgrid, cdf, sc.db, draws='counter', **kw)          # frame 2 i + v
    stream = particles.expected_records(sims, dgrid, cdf, sc.db, **kw)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        cases.set_rig(rh, opt)
        rh.set_particle_draws('counter')
        for chunks in (1, 2):
            rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
            cnt = _check(rh, sims, want, 'rig, %d chunks' % chunks)
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, 0)
        small, cnt_small = rh.generate_drops(sims, H, W, cap=max(len(want[1]) // 2, 1))
        assert np.array_equal(cnt_small, cnt)
        assert len(small[1]) == len(want[1]) // 2 and small[1].tobytes() == want[1][:len(small[1])].tobytes()
        # view 1 alone: the same bits per view
        cases.set_rig(rh, opt, active=[1])
        got, _ = rh.generate_drops(particles.rig_run_sims(sims1, inst, 1), H, W)
        for i in range(len(inst)):
            cases.same_bytes(got[i], want[2 * i + 1], 'active [1]: instant %d' % i)
        cases.set_rig(rh, opt)
        rh.set_particle_draws('stream')
        _check(rh, sims, stream, 'rig, stream again')
    finally:
        rh.close()


def test_counter_mode_launches_no_draws_kernel(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.kitti()
    rh = cases.rain_hip(sc)
    try:
        rh.profile(True)
        for name, (sims, dgrid, cdf, kw) in (('k_particles', cases.iid_run(opt)), ('k_field_particles', cases.field_run(opt))):
            rh.set_particle_tables(dgrid, cdf)
            rh.set_particle_model(kw['model'], kw.get('cam_hz', 0.0))
            for draws, launches in (('counter', 0), ('stream', 1)):
                rh.set_particle_draws(draws)
                rh.profile_reset()
                rh.generate_drops(sims, H, W)
                stats = rh.profile_read()
                assert stats[name][0] >= 1, (name, draws, stats)
                assert stats.get('k_particle_draws', (0, 0.0))[0] == launches, (name, draws, stats)
    finally:
        rh.close()


def test_invalid_combinations_are_refused(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    sims, dgrid, cdf, _ = cases.iid_run(cases.kitti())
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        with pytest.raises(RuntimeError, match='unknown mode'):
            rh._check(rh.lib.rr_set_particle_draws(rh.h, 2), 'rr_set_particle_draws')
        with pytest.raises(ValueError, match='particle draws'):
            rh.set_particle_draws('philox')
        # angular noise first, then counter draws
        rh.set_particle_noise(2.0, 1.0, [0], [0])
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.set_particle_draws('counter')
        rh.set_particle_noise(0.0, 0.0)
        # counter draws first, then angular noise; a record that names a run entry
        rh.set_particle_draws('counter')
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.set_particle_noise(2.0, 1.0, [0], [0])
        bad = sims.copy()
        bad['run_pos'] = 1
        with pytest.raises(RuntimeError, match='run_pos'):
            rh.generate_drops(bad, H, W)
        got, cnt = rh.generate_drops(sims, H, W)                # the context still works
        assert int(cnt[0]) > 100
    finally:
        rh.close()


def test_rain_augment_renders_the_host_statements_records(built, streaks_db):
    """RainAugment(draws='counter'), B = 2, bytes, KITTI, 25 mm/hr, against rr_pipeline_submit fed expected_records(draws='counter')
    as host tables: image bytes and mask equal (tests/test_gpu_augment.py makes this comparison for the stream mode)."""
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', draws='counter')
    stream_aug = None
    try:
        Hf, Wf = aug.frame_size()
        assert (Hf, Wf) == (H, W)
        bgr, depth = _scene(2, H, W, seed=40)
        idx = [4, 11]
        p = aug.plan(25, idx)
        assert p['draws'] == 'counter'
        want = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, draws='counter')
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
        # the stream mode renders other pixels from the same call (another texture per drop)
        stream_aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training')
        rainy_s, _ = stream_aug(_planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV), 25, idx)
        assert not np.array_equal(rainy_s.cpu().numpy(), rainy)
    finally:
        aug.close()
        if stream_aug is not None:
            stream_aug.close()
