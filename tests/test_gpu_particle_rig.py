"""GPU tier: the RIG particle model on the device (rr_set_particle_rig, k_rig_particles).

  1. device records == the host statement (tools/particles.py expected_records(model='rig')), bit for bit, counts included: KITTI
     stereo at two intensities, Cityscapes stereo at render scale 2, a six-view ring at nuScenes size; every split of an instant's
     slots over workgroups (RR_OPT_FIELD_CHUNKS); a subset and a permutation of the active views; 1 instant and 64;
  2. rr_render_frames with sim records renders exactly the host statement's records;
  3. RainAugment(particle_model='rig') on [B, V] == the views one per call == the files of `main.py --rig_view v` runs, one rank
     and two ranks on the one GPU;
  4. the i.i.d. and the field model's bits do not move after a rig has been set and unset on the same context;
  5. the library's refusals."""
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


@pytest.mark.parametrize("dataset,rs,rate,rig", cases.CONFIGS, ids=cases.IDS)
def test_device_records_equal_host_statement(tmp_path, built, dataset, rs, rate, rig):
    sc = h.Scene(tmp_path, 64, 96, 10)                       # (only its streak database is used: the texture ratios)
    opt = cases.options(dataset, sim_steps={"cam_motion": np.array([30.0])})
    hz = opt['cam_hz']
    V = len(rig)
    sims1, dgrid, cdf = particles.sim_frames(opt, rate, 1, render_scale=rs, seed=1234 + 2 ** 40, model='rig', rig=rig)
    inst = [0, 1, 2 ** 31 + 5]
    sims = particles.rig_run_sims(sims1, inst, V)
    want = particles.expected_records(sims, dgrid, cdf, sc.db, model='rig', cam_hz=hz, rig=rig)          # frame i * V + v
    W, H = opt["cam_CCD_WH"][0] // rs, opt["cam_CCD_WH"][1] // rs
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        cases.set_rig(rh, opt, rig)
        for chunks in (0, 1, 2, 64):
            rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
            got, cnt = rh.generate_drops(sims, H, W)
            for k in range(len(sims)):
                assert int(cnt[k]) == len(want[k]) > 100
                cases.same_bytes(got[k], want[k], 'instant %d view %d, %d chunks' % (k // V, k % V, chunks))
            alone, _ = rh.generate_drops(sims[V:2 * V], H, W)                  # a batch of one instant
            for v in range(V):
                cases.same_bytes(alone[v], want[V + v], 'instant 1 alone, view %d, %d chunks' % (v, chunks))
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, 0)
        # a subset of the views, and a permutation: the same tables per (instant, view), nothing else moves
        sub = [V - 1] if V == 2 else [4, 1, 2]
        cases.set_rig(rh, opt, rig, active=sub)
        got, _ = rh.generate_drops(particles.rig_run_sims(sims1, inst, len(sub)), H, W)
        for i in range(len(inst)):
            for a, v in enumerate(sub):
                cases.same_bytes(got[i * len(sub) + a], want[i * V + v], 'active %r: instant %d view %d' % (sub, i, v))
        perm = list(range(V))[::-1]
        cases.set_rig(rh, opt, rig, active=perm)
        got, _ = rh.generate_drops(sims, H, W)
        for i in range(len(inst)):
            for a, v in enumerate(perm):
                cases.same_bytes(got[i * V + a], want[i * V + v], 'active %r: instant %d view %d' % (perm, i, v))
        # a capacity below the drop count: the count still tells, the records that fit are the first ones
        cases.set_rig(rh, opt, rig)
        small, cnt_small = rh.generate_drops(sims, H, W, cap=max(len(want[1]) // 2, 1))
        assert np.array_equal(cnt_small, cnt)
        assert small[1].tobytes() == want[1][:len(small[1])].tobytes()
        if dataset == 'kitti' and rate == 25:                                  # 64 instants in one batch
            many = particles.rig_run_sims(sims1, 100 + np.arange(64), V)
            want64 = particles.expected_records(many, dgrid, cdf, sc.db, model='rig', cam_hz=hz, rig=rig)
            got, cnt64 = rh.generate_drops(many, H, W)
            for k in range(len(many)):
                assert int(cnt64[k]) == len(want64[k])
                cases.same_bytes(got[k], want64[k], 'batch of 64 instants: frame %d' % k)
    finally:
        rh.close()


def test_frame_path_renders_the_host_statements_records(tmp_path, built):
    """rr_render_frames with rr_frame_in.sim under the rig model (KITTI stereo) against the same call fed expected_records:
    count, drop status, mask and image identical."""
    opt = cases.options('kitti')
    W, H = opt["cam_CCD_WH"]
    rig = cases.KITTI_STEREO
    sc = h.Scene(tmp_path, H, W, 10)
    sims, dgrid, cdf = particles.sim_frames(opt, 100, 1, seed=77, model='rig', rig=rig)
    sims = particles.rig_run_sims(sims, [5, 6], 2)
    want = particles.expected_records(sims, dgrid, cdf, sc.db, model='rig', cam_hz=opt['cam_hz'], rig=rig)
    bg, env = sc.frame_inputs(0)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        cases.set_rig(rh, opt, rig)
        outs = rh.render_frames([dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, sim=sims[k]) for k in range(4)])
        refs = rh.render_frames([dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=want[k]) for k in range(4)])
        with pytest.raises(RuntimeError, match='multiple'):
            rh.render_frames([dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, sim=sims[k]) for k in range(3)])
    finally:
        rh.close()
    for k in range(4):
        n = outs[k]['n_drops']
        assert n == len(want[k]) > 100
        assert np.array_equal(outs[k]['status'][:n], refs[k]['status'])
        assert np.array_equal(outs[k]['mask'], refs[k]['mask']) and np.array_equal(outs[k]['image_u8'], refs[k]['image_u8'])
        assert outs[k]['mask'].max() > 0
    assert not np.array_equal(outs[0]['mask'], outs[1]['mask']) and not np.array_equal(outs[0]['mask'], outs[2]['mask'])


def test_other_models_bits_do_not_move(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    hz = opt['cam_hz']
    W, H = opt["cam_CCD_WH"]
    rig = cases.KITTI_STEREO
    rh = cases.rain_hip(sc)
    try:
        for model in ('iid', 'field'):
            sims, dgrid, cdf = particles.sim_frames(opt, 25, 1, seed=9, model=model)
            sims = np.concatenate([sims, sims])
            sims['draw_seed'] = [3, 4]
            want = particles.expected_records(sims, dgrid, cdf, sc.db, model=model, cam_hz=hz)
            rh.set_particle_tables(dgrid, cdf)
            rh.set_particle_model(model, hz)
            before, cb = rh.generate_drops(sims, H, W)
            cases.set_rig(rh, opt, rig)
            through, _ = rh.generate_drops(sims, H, W)           # (the other model's table under the rig model: other rain)
            rh.set_particle_model(model, hz)
            after, ca = rh.generate_drops(sims, H, W)
            for k in range(2):
                assert int(cb[k]) == int(ca[k]) == len(want[k])
                assert before[k].tobytes() == after[k].tobytes() == want[k].tobytes()
                assert through[k].tobytes() != before[k].tobytes()
    finally:
        rh.close()


def test_invalid_combinations_are_refused(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    rig = cases.KITTI_STEREO
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1, model='rig', rig=rig)
    sims = particles.rig_run_sims(sims, [0, 1], 2)
    views, box = rig.as_records(), rig.box(particles.FrameCamera(opt, 0))
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        with pytest.raises(RuntimeError, match='needs a rig first'):
            rh.set_particle_model('rig', 10.0)
        nine = np.concatenate([views] * 5)[:9]
        for bad in (views[:0], nine):
            with pytest.raises(RuntimeError, match='n_views'):
                rh.set_particle_rig(bad, box)
        skew = views.copy()
        skew['R'][1][0] = 1.0 + 1e-6
        with pytest.raises(RuntimeError, match='orthonormal'):
            rh.set_particle_rig(skew, box)
        mirror = views.copy()
        mirror['R'][0][8] = -1.0
        with pytest.raises(RuntimeError, match='orthonormal'):
            rh.set_particle_rig(mirror, box)
        for bad in ([0, 0], [2], [-1], [0, 1, 0]):
            with pytest.raises(RuntimeError, match='active'):
                rh.set_particle_rig(views, box, active=bad)
        for bad in ((0.0, box[1], 0.0), (box[0], -1.0, 0.0), (box[0], box[1], -0.1), (float('nan'), box[1], 0.0), (box[0], float('inf'), 0.0)):
            with pytest.raises(RuntimeError, match='box'):
                rh.set_particle_rig(views, bad)
        rh.set_particle_rig(views, box)
        for hz in (0.0, float('nan')):
            with pytest.raises(RuntimeError, match='cam_hz'):
                rh.set_particle_model('rig', hz)
        rh.set_particle_noise(2.0, 1.0, [0], [0])
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.set_particle_model('rig', 10.0)
        rh.set_particle_noise(0.0, 0.0)
        rh.set_particle_model('rig', 10.0)
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.set_particle_noise(2.0, 1.0, [0], [0])
        with pytest.raises(RuntimeError, match='multiple'):
            rh.generate_drops(sims[:3], 375, 1242)
        odd = sims.copy()
        odd['speed_mps'][1] += 1.0
        with pytest.raises(RuntimeError, match='must agree'):
            rh.generate_drops(odd, 375, 1242)
        noisy = sims.copy()
        noisy['run_pos'] = 1
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.generate_drops(noisy, 375, 1242)
        seeds = sims.copy()
        seeds['draw_seed'] = [5, 6, 7, 8]                         # draw_seed may differ inside an instant
        got, cnt = rh.generate_drops(seeds, 375, 1242)
        assert all(int(c) > 100 for c in cnt)
    finally:
        rh.close()


def test_driver_runs_per_view_and_the_augmenter_agree(tmp_path, built, monkeypatch):
    """A short KITTI-sized sequence: `main.py --particle_model rig --rig stereo:0.54 --rig_view v` for v = 0, 1 as one rank, and view
    1 once more as two ranks on GPU 0 (byte-identical folders); RainAugment(rig) on the [B, V] clip (uint8) gives the RGB bytes of
    both runs' files, and the same as the views rendered one per call."""
    tmp = str(tmp_path)
    H, W, n = 375, 1242, 4
    src = os.path.join(tmp, 'source')
    h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), n, H, W, depth_m=None)
    streaks_db = os.path.join(tmp, 'rainstreakdb')
    h.synthetic.write_streak_db(streaks_db)
    main = importlib.import_module('rain-rendering_amd.main')
    common = ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', streaks_db, '-i', '25', '--noverbose',
              '--device_particles', '--particle_model', 'rig', '--rig', 'stereo:0.54']
    monkeypatch.setenv('RAIN_BATCH', '3')                              # two batches, the second ragged
    for v in (0, 1):
        gen = main.main(common + ['--rig_view', str(v), '--output', os.path.join(tmp, 'view%d' % v)])
        assert len(gen.stats) == n and all(s['drops'] > 100 for s in gen.stats)
    with pytest.raises(SystemExit, match='go together'):
        main.main(common[:-2] + ['--output', os.path.join(tmp, 'outx')])
    env = dict(os.environ, RAIN_DEVICE='0', RAIN_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', RAIN_BATCH='2')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(cases.free_port()), os.path.join(h.ROOT, 'rain-rendering_amd', 'main.py')] + common +
                       ['--rig_view', '1', '--output', os.path.join(tmp, 'view1_2ranks'), '--conflict_strategy', 'rename_folder'],
                       env=env, cwd=h.ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-3000:], r.stderr.decode()[-3000:])
    sub = os.path.join('kitti', 'data_object', 'training', 'rain', '25mm')
    names = ['%06d.png' % i for i in range(n)]
    for kind in ('rainy_image', 'rain_mask'):
        a, b = os.path.join(tmp, 'view1', sub, kind), os.path.join(tmp, 'view1_2ranks', sub, kind)
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == names
        for f in names:
            assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), (kind, f)
            assert open(os.path.join(a, f), 'rb').read() != open(os.path.join(tmp, 'view0', sub, kind, f), 'rb').read(), (kind, f)
    img_dir = os.path.join(src, 'kitti', 'data_object', 'training', 'image_2')
    rgb = np.stack([np.array(Image.open(os.path.join(img_dir, f)).convert('RGB')) for f in names])
    depth = np.stack([np.array(Image.open(os.path.join(img_dir, 'depth', f))).astype(np.float32) / 256. for f in names])
    files = np.stack([np.stack([np.array(Image.open(os.path.join(tmp, 'view%d' % v, sub, 'rainy_image', f)))[..., :3] for v in (0, 1)])
                      for f in names])                                  # [n, V, H, W, 3]
    kw = dict(streaks_db=streaks_db, sequence='data_object/training', particle_model='rig', rig=cases.KITTI_STEREO)
    aug = augment.RainAugment('kitti', **kw)
    right = augment.RainAugment('kitti', views=[1], **kw)
    try:
        img8 = torch.from_numpy(rgb.transpose(0, 3, 1, 2).copy()).to(DEV)
        dep = torch.from_numpy(depth).to(DEV)
        both = torch.stack([img8, img8], dim=1)                         # the synthetic set has one camera: both views start from its images
        dep2 = torch.stack([dep, dep], dim=1)
        clip = np.arange(n)
        rainy, mask = aug(both, dep2, 25, clip)
        assert tuple(rainy.shape) == (n, 2, 3, H, W) and tuple(mask.shape) == (n, 2, 1, H, W)
        assert np.array_equal(rainy.cpu().numpy().transpose(0, 1, 3, 4, 2), files)
        assert not torch.equal(mask[:, 0], mask[:, 1]) and all(float(mask[i, v].max()) > 0 for i in range(n) for v in (0, 1))
        r1, m1 = right(both[:, 1:], dep2[:, 1:].unsqueeze(2), 25, clip)              # one view per call, depth as [B, V, 1, H, W]
        assert torch.equal(r1, rainy[:, 1:]) and torch.equal(m1, mask[:, 1:])
        r2, m2 = aug(both[2:3], dep2[2:3], 25, [2])                                  # random access
        assert torch.equal(r2, rainy[2:3]) and torch.equal(m2, mask[2:3])
    finally:
        aug.close()
        right.close()
