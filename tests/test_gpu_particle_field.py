"""GPU tier: the FIELD particle model on the device (rr_set_particle_model, k_field_particles).

  1. device records == the host statement (tools/particles.py expected_records(model='field')), bit for bit, counts included,
     at KITTI, Cityscapes and nuScenes sizes and two intensities, for every split of a frame's slots over workgroups
     (RR_OPT_FIELD_CHUNKS); through rr_generate_drops and through the frame path (rr_frame_in.sim);
  2. `main.py --device_particles --particle_model field` as one rank and as two ranks sharing GPU 0: byte-identical folders;
     RainAugment(particle_model='field') on the clip == the files of that run, uint8 and float32;
  3. the default model's bits do not move when the field model is selected and de-selected on the same context;
  4. invalid combinations are RR_E_ARG with a message."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import helpers as h
import particle_cases as cases

pytestmark = pytest.mark.gpu

particles = importlib.import_module('rain-rendering_amd.tools.particles')
augment = importlib.import_module('rain-rendering_amd.augment')

DEV = torch.device('cuda', 0)
CAMS = {'kitti': None, 'cityscapes': None, 'nuscenes': h.NUSCENES}


@pytest.mark.parametrize("dataset,rs", [('kitti', 1), ('cityscapes', 2), ('nuscenes', 1)])
@pytest.mark.parametrize("rate", [25, 100])
def test_device_records_equal_host_statement(tmp_path, built, dataset, rs, rate):
    sc = h.Scene(tmp_path, 64, 96, 10)                       # (only its streak database is used: the texture ratios)
    opt = cases.options(dataset, sim_steps={"cam_motion": np.array([30.0, 50.0, 0.0])})
    sims, dgrid, cdf = particles.sim_frames(opt, rate, 3, render_scale=rs, seed=1234 + 2 ** 40, model='field')
    sims = particles.field_run_sims(sims, [0, 1, 17, 2 ** 31 + 5, 4000000000])
    hz = opt['cam_hz']
    want = particles.expected_records(sims, dgrid, cdf, sc.db, model='field', cam_hz=hz)
    W, H = opt["cam_CCD_WH"][0] // rs, opt["cam_CCD_WH"][1] // rs
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        rh.set_particle_model('field', hz)
        for chunks in (0, 1, 3, 64):
            rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
            got, cnt = rh.generate_drops(sims, H, W)
            for k in range(len(sims)):
                assert int(cnt[k]) == len(want[k]) > 100
                cases.same_bytes(got[k], want[k], 'frame %d, %d chunks' % (k, chunks))
            # a frame alone, and in another order: the same bits (no state, no dependence on the batch)
            alone, _ = rh.generate_drops(sims[3:4], H, W)
            cases.same_bytes(alone[0], want[3], 'frame 3 alone, %d chunks' % chunks)
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, 0)
        back, _ = rh.generate_drops(sims[::-1], H, W)
        for k in range(len(sims)):
            cases.same_bytes(back[len(sims) - 1 - k], want[k], 'frame %d, reversed batch' % k)
        # a capacity below the drop count: the count still tells, the records that fit are the first ones
        small, cnt_small = rh.generate_drops(sims, H, W, cap=max(len(want[0]) // 2, 1))
        assert np.array_equal(cnt_small, cnt)
        assert small[0].tobytes() == want[0][:len(small[0])].tobytes()
    finally:
        rh.close()
    assert set(np.concatenate([w['type'] for w in want])) == {0, 1, 2}


@pytest.mark.parametrize("dataset,rs,rate", [('kitti', 1, 100), ('cityscapes', 2, 25), ('nuscenes', 1, 25)])
def test_frame_path_renders_the_host_statements_records(tmp_path, built, dataset, rs, rate):
    """rr_render_frames with rr_frame_in.sim under the field model against the same call fed expected_records: count, drop
    status, mask and image identical."""
    opt = cases.options(dataset)
    W, H = opt["cam_CCD_WH"][0] // rs, opt["cam_CCD_WH"][1] // rs
    sc = h.Scene(tmp_path, H, W, 10, **({'cam': CAMS[dataset]} if CAMS[dataset] is not None else {}))
    sims, dgrid, cdf = particles.sim_frames(opt, rate, 1, render_scale=rs, seed=77, model='field')
    sims = particles.field_run_sims(sims, [5, 6])
    want = particles.expected_records(sims, dgrid, cdf, sc.db, model='field', cam_hz=opt['cam_hz'])
    bg, env = sc.frame_inputs(0)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        rh.set_particle_model('field', opt['cam_hz'])
        outs = rh.render_frames([dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, sim=sims[k]) for k in range(2)])
        refs = rh.render_frames([dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=want[k]) for k in range(2)])
    finally:
        rh.close()
    for k in range(2):
        n = outs[k]['n_drops']
        assert n == len(want[k]) > 100
        assert np.array_equal(outs[k]['status'][:n], refs[k]['status'])
        assert np.array_equal(outs[k]['mask'], refs[k]['mask']) and np.array_equal(outs[k]['image_u8'], refs[k]['image_u8'])
        assert outs[k]['mask'].max() > 0
    assert not np.array_equal(outs[0]['mask'], outs[1]['mask'])


def test_default_models_bits_do_not_move(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    rh = cases.rain_hip(sc)
    try:
        for dataset, rs in (('kitti', 1), ('cityscapes', 2), ('nuscenes', 1)):
            opt = cases.options(dataset)
            sims, dgrid, cdf = particles.sim_frames(opt, 25, 1, render_scale=rs, seed=9)
            want = particles.expected_records(sims, dgrid, cdf, sc.db)
            W, H = opt["cam_CCD_WH"][0] // rs, opt["cam_CCD_WH"][1] // rs
            rh.set_particle_tables(dgrid, cdf)
            before, cb = rh.generate_drops(sims, H, W)
            rh.set_particle_model('field', opt['cam_hz'])
            field, cf = rh.generate_drops(sims, H, W)
            rh.set_particle_model('iid')
            after, ca = rh.generate_drops(sims, H, W)
            assert int(cb[0]) == int(ca[0]) == len(want[0]) and before[0].tobytes() == after[0].tobytes() == want[0].tobytes()
            assert field[0].tobytes() != before[0].tobytes()
    finally:
        rh.close()


def test_invalid_combinations_are_refused(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1, model='field')
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        for hz in (0.0, -10.0, float('nan'), float('inf')):
            with pytest.raises(RuntimeError, match='cam_hz'):
                rh.set_particle_model('field', hz)
        with pytest.raises(RuntimeError, match='unknown model'):
            rh._check(rh.lib.rr_set_particle_model(rh.h, 7, 10.0), 'rr_set_particle_model')
        with pytest.raises(ValueError, match='particle model'):
            rh.set_particle_model('brownian', 10.0)
        # angular noise first, then the field model
        rh.set_particle_noise(2.0, 1.0, [0], [0])
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.set_particle_model('field', 10.0)
        rh.set_particle_noise(0.0, 0.0)
        # the field model first, then angular noise; a record that names a run entry
        rh.set_particle_model('field', 10.0)
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.set_particle_noise(2.0, 1.0, [0], [0])
        bad = sims.copy()
        bad['run_pos'] = 1
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.generate_drops(bad, 375, 1242)
        got, cnt = rh.generate_drops(sims, 375, 1242)           # the context still works
        assert int(cnt[0]) > 100
    finally:
        rh.close()


def _pipeline_f32(aug, p, bgr, depth):
    """rr_pipeline_submit under the field model on the records of plan `p`, float32 interleaved BGR inputs: image_u8 RGB [n, H, W, 3]
    (the call RainAugment promises the bits of; tests/test_gpu_augment.py does the same for the default model)."""
    imgops = importlib.import_module('rain-rendering_amd.common.imgops')
    envmod = importlib.import_module('rain-rendering_amd.common.envmap')
    n, H, W = bgr.shape[:3]
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(aug.db.streaks_light)
        rh.set_camera(h.hb.make_camera(aug.focal, aug.f_number, aug.exposure))
        rh.set_prepass_kernels(imgops.gaussian_kernel(25, 25), imgops.gaussian_kernel(15, 0))
        rh.set_particle_tables(p['d_grid'], p['cdf'])
        rh.set_particle_model(p['particle_model'], p['cam_hz'])
        we = rh.set_envmap_geometry(H, W, *envmod.EnvironmentMapGenerator(aug.focal, W, H).device_tables(H, W))
        rh.set_solid_angles(h.solid_angle.get_solid_angles(np.empty((H, we, 0))))
        frames = [dict(bg=np.ascontiguousarray(bgr[i]), depth=np.ascontiguousarray(depth[i]), fog=tuple(p['fog'][i]), omega=None,
                       sim=p['sims'][i:i + 1].copy(), drops_cap=p['drops_cap']) for i in range(n)]
        outs = [dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W))) for _ in range(n)]
        rh.pipeline_submit(0, frames, outs)
        while not rh.pipeline_wait(0):
            rh.pipeline_submit(0, frames, outs)
    finally:
        rh.close()
    return np.stack([o['image_u8'] for o in outs])


def test_driver_one_rank_two_ranks_and_the_augmenter_agree(tmp_path, built, monkeypatch):
    """A short KITTI-sized sequence: the field-model run as one rank and as two ranks on GPU 0 writes byte-identical folders
    (every rank makes its own frames from the frame index alone); RainAugment(particle_model='field') on the clip gives the
    pixels of the files; the --noise_std combination is refused; and the run differs from the default model's.

    What "the pixels of the files" means is what RainAugment gives for the default model.  From uint8 images: the bytes of the
    PNG, bit for bit.  From float32 images (byte / 255, as ToTensor makes them): the bits of rr_pipeline_frames fed those
    float32 values -- and the files only within the image contract of +-1 LSB, because the library's pre-pass starts from other
    bits when it is handed bytes.  Measured on an MI355X on this clip (6 KITTI frames, 8 383 500 values): the default model's
    float32 result differs from its files in 35 values, the field model's in 18, each by 1 LSB; both uint8 results are the
    files' bytes.  So float32 is held to the pipeline's bits and to +-1 LSB of the files, uint8 to the files' bits."""
    tmp = str(tmp_path)
    H, W, n = 375, 1242, 6
    src = os.path.join(tmp, 'source')
    h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), n, H, W, depth_m=None)
    streaks_db = os.path.join(tmp, 'rainstreakdb')
    h.synthetic.write_streak_db(streaks_db)
    main = importlib.import_module('rain-rendering_amd.main')
    common = ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', streaks_db, '-i', '25', '--noverbose',
              '--device_particles']
    monkeypatch.setenv('RAIN_BATCH', '4')                              # two batches, the second ragged
    gen = main.main(common + ['--particle_model', 'field', '--output', os.path.join(tmp, 'out1')])
    assert len(gen.stats) == n and all(s['drops'] > 100 for s in gen.stats)
    main.main(common + ['--output', os.path.join(tmp, 'out0')])
    with pytest.raises(SystemExit, match='noise_std'):
        main.main(common + ['--particle_model', 'field', '--noise_std', '2', '--output', os.path.join(tmp, 'outn')])
    env = dict(os.environ, RAIN_DEVICE='0', RAIN_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', RAIN_BATCH='2')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(cases.free_port()), os.path.join(h.ROOT, 'rain-rendering_amd', 'main.py')] + common +
                       ['--particle_model', 'field', '--output', os.path.join(tmp, 'out2'), '--conflict_strategy', 'rename_folder'],
                       env=env, cwd=h.ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-3000:], r.stderr.decode()[-3000:])
    sub = os.path.join('kitti', 'data_object', 'training', 'rain', '25mm')
    names = ['%06d.png' % i for i in range(n)]
    for kind in ('rainy_image', 'rain_mask'):
        a, b = os.path.join(tmp, 'out1', sub, kind), os.path.join(tmp, 'out2', sub, kind)
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == names
        for f in names:
            assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), (kind, f)
        differ = [open(os.path.join(a, f), 'rb').read() != open(os.path.join(tmp, 'out0', sub, kind, f), 'rb').read() for f in names]
        assert all(differ), kind                                    # another model, another rain
    # the augmenter on the clip
    img_dir = os.path.join(src, 'kitti', 'data_object', 'training', 'image_2')
    rgb = np.stack([np.array(Image.open(os.path.join(img_dir, f)).convert('RGB')) for f in names])
    depth = np.stack([np.array(Image.open(os.path.join(img_dir, 'depth', f))).astype(np.float32) / 256. for f in names])
    files = np.stack([np.array(Image.open(os.path.join(tmp, 'out1', sub, 'rainy_image', f)))[..., :3] for f in names])
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', particle_model='field')
    try:
        img8 = torch.from_numpy(rgb.transpose(0, 3, 1, 2).copy()).to(DEV)
        dep = torch.from_numpy(depth).to(DEV)
        clip = np.arange(n)
        rainy8, mask8 = aug(img8, dep, 25, clip)
        f32 = (rgb.astype(np.float64) / 255.0).astype(np.float32)        # the bytes as ToTensor hands them over (correctly rounded)
        rainyf, maskf = aug(torch.from_numpy(f32.transpose(0, 3, 1, 2).copy()).to(DEV), dep, 25, clip)
        assert np.array_equal(rainy8.cpu().numpy().transpose(0, 2, 3, 1), files)
        gotf = rainyf.cpu().numpy().transpose(0, 2, 3, 1)
        pipe = _pipeline_f32(aug, aug.plan(25, clip), f32[..., ::-1], depth)
        assert np.array_equal(gotf, pipe.astype(np.float32) / np.float32(255.0))
        lsb = np.abs(np.rint(gotf.astype(np.float64) * 255.0) - files)
        print('float32 clip against the files: %d of %d values differ, largest difference %g LSB' % ((lsb != 0).sum(), lsb.size, lsb.max()))
        assert lsb.max() <= 1
        assert torch.equal(mask8, maskf) and all(float(mask8[i].max()) > 0 for i in range(n))
        # random access: the clip's frames one by one, in another order
        for i in (4, 1):
            r1, m1 = aug(img8[i:i + 1], dep[i:i + 1], 25, [i])
            assert torch.equal(r1, rainy8[i:i + 1]) and torch.equal(m1, mask8[i:i + 1])
    finally:
        aug.close()
