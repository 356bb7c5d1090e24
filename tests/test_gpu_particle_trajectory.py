"""GPU tier: the rig particle model under a camera trajectory on the device (rr_set_particle_trajectory, k_rig_particles<.., TRAJ>).

  1. device records == the host statement (tools/particles.py expected_records(trajectory=)), bit for bit, counts included: KITTI
     stereo and a single camera on an arc, a table whose rows are not consecutive time indices, an instant repeated inside the
     batch, a pose 1e5 m from the origin, every split of an instant's slots over workgroups (the count pass and the store pass
     must read the same row), a subset and a permutation of the active views, a capacity below the count;
  2. a trajectory whose two ends coincide gives the rig model's bytes for those views on the same context; after the trajectory
     is turned off the rig, field and i.i.d. models give what they gave before;
  3. counter draws and the streak jitter: bit for bit, and a slot seen in two views and in two consecutive frames of one life
     keeps its texture pick and its tilt;
  4. RainAugment(trajectory=) on [B = 2, V = 2] == the files of `main.py --trajectory` runs per view;
  5. the library's refusals, each with its message."""
import importlib
import os

import numpy as np
import pytest
import torch
from PIL import Image

import helpers as h
import particle_cases as cases

pytestmark = pytest.mark.gpu

particles = importlib.import_module('rain-rendering_amd.tools.particles')
rigmod = importlib.import_module('rain-rendering_amd.rig')
trajmod = importlib.import_module('rain-rendering_amd.trajectory')
augment = importlib.import_module('rain-rendering_amd.augment')

DEV = torch.device('cuda', 0)


def _arc_with_a_far_pose():
    """Poses 0 .. 8: the arc (10 m/s, 20 deg/s, 10 Hz); poses 9 and 10: 1e5 m away, a metre apart, pitched."""
    far = np.array([6e4, 0.0, -8e4])
    return trajmod.Trajectory(np.array(cases.arc_poses(9) + [cases.pose(140.0, 6.0, far), cases.pose(142.0, 6.5, far + np.array([0.4, 0.02, 0.9]))]), 10.0)


@pytest.mark.parametrize("rig", [cases.KITTI_STEREO, cases.MONO], ids=['kitti25-stereo', 'kitti25-mono'])
def test_device_records_equal_host_statement(tmp_path, built, rig):
    sc = h.Scene(tmp_path, 64, 96, 10)                       # (only its streak database is used: the texture ratios)
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([30.0])})
    hz = opt['cam_hz']
    V = len(rig)
    traj = _arc_with_a_far_pose()
    sims1, dgrid, cdf = particles.sim_frames(opt, 25, 1, seed=1234 + 2 ** 40, model='rig', rig=rig, trajectory=traj)
    rows = [0, 1, 5, 7, 9]                                   # the table's time indices: not consecutive
    inst = [0, 1, 7, 1, 9]                                   # instant 1 twice in the batch; 9 is the far pose
    sims = particles.rig_run_sims(sims1, inst, V)
    kw = dict(model='rig', cam_hz=hz, rig=rig, trajectory=traj)
    want = particles.expected_records(sims, dgrid, cdf, sc.db, **kw)          # frame i * V + v
    assert all(want[V + v].tobytes() == want[3 * V + v].tobytes() for v in range(V)) and want[0].tobytes() != want[V].tobytes()
    W, H = opt["cam_CCD_WH"]
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        cases.set_trajectory(rh, rig, traj, opt, hz, rows=rows)
        for chunks in (0, 1, 2, 64):
            rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, chunks)
            got, cnt = rh.generate_drops(sims, H, W)
            for k in range(len(sims)):
                assert int(cnt[k]) == len(want[k]) > 100, (k, chunks, int(cnt[k]), len(want[k]))
                cases.same_bytes(got[k], want[k], 'instant %d view %d, %d chunks' % (inst[k // V], k % V, chunks))
            alone, _ = rh.generate_drops(sims[2 * V:3 * V], H, W)                # a batch of one instant: row 3 of the table
            for v in range(V):
                cases.same_bytes(alone[v], want[2 * V + v], 'instant 7 alone, view %d, %d chunks' % (v, chunks))
        rh.set_option(h.hb.RR_OPT_FIELD_CHUNKS, 0)
        if V == 2:                                               # a subset of the views, and a permutation
            cases.set_trajectory(rh, rig, traj, opt, hz, active=[1], rows=rows)
            got, _ = rh.generate_drops(particles.rig_run_sims(sims1, inst, 1), H, W)
            for i in range(len(inst)):
                cases.same_bytes(got[i], want[i * V + 1], 'active [1]: instant %d' % inst[i])
            cases.set_trajectory(rh, rig, traj, opt, hz, active=[1, 0], rows=rows)
            got, _ = rh.generate_drops(sims, H, W)
            for i in range(len(inst)):
                for a, v in enumerate([1, 0]):
                    cases.same_bytes(got[i * V + a], want[i * V + v], 'active [1, 0]: instant %d view %d' % (inst[i], v))
            cases.set_trajectory(rh, rig, traj, opt, hz, rows=rows)
        # a capacity below the drop count: the count still tells, the records that fit are the first ones
        small, cnt_small = rh.generate_drops(sims, H, W, cap=max(len(want[1]) // 2, 1))
        assert np.array_equal(cnt_small, cnt)
        assert small[1].tobytes() == want[1][:len(small[1])].tobytes()
    finally:
        rh.close()


def test_coincident_ends_and_turning_it_off(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([30.0])})     # speed_mps stays in the formula: a drift of the world
    hz = opt['cam_hz']
    W, H = opt["cam_CCD_WH"]
    rig = cases.KITTI_STEREO
    cam = particles.FrameCamera(opt, 0)
    still = trajmod.Trajectory(np.array([cases.pose(37.0, 5.0, (1e3, 0.4, -2e3))] * 3), 10.0)
    po = still.compose(rig, cam.exposure)
    assert po['R0'].tobytes() == po['R1'].tobytes() and po['c0'].tobytes() == po['c1'].tobytes()
    box = still.box(rig, cam)
    seen = rigmod.Rig([(po['R0'][1, v].reshape(3, 3), po['c0'][1, v]) for v in range(2)])      # the composed views as a rig of their own
    sims1, dgrid, cdf = particles.sim_frames(opt, 25, 1, seed=5, model='rig', rig=still.bind(rig))
    assert float(sims1['speed_mps'][0]) > 8.0
    sims = particles.rig_run_sims(sims1, [1, 2], 2)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        rh.set_particle_rig(seen.as_records(), box)
        rh.set_particle_model('rig', hz)
        plain, cp = rh.generate_drops(sims, H, W)
        rh.set_particle_rig(rig.as_records(), box)
        rh.set_particle_trajectory(po)
        through, ct = rh.generate_drops(sims, H, W)
        assert np.array_equal(cp, ct) and all(int(c) > 100 for c in cp)
        for k in range(4):
            assert plain[k].tobytes() == through[k].tobytes(), k
        # the rig model proper, before the trajectory and after it is turned off
        rh.set_particle_trajectory(None)
        rsims, rgrid, rcdf = particles.sim_frames(opt, 25, 1, seed=5, model='rig', rig=rig)
        rsims = particles.rig_run_sims(rsims, [1, 2], 2)
        rwant = particles.expected_records(rsims, rgrid, rcdf, sc.db, model='rig', cam_hz=hz, rig=rig)
        rh.set_particle_tables(rgrid, rcdf)
        rh.set_particle_rig(rig.as_records(), rig.box(cam))
        before, _ = rh.generate_drops(rsims, H, W)
        rh.set_particle_trajectory(_arc_with_a_far_pose().compose(rig, cam.exposure))
        moved, _ = rh.generate_drops(rsims, H, W)
        rh.set_particle_trajectory(None)
        after, _ = rh.generate_drops(rsims, H, W)
        for k in range(4):
            assert before[k].tobytes() == after[k].tobytes() == rwant[k].tobytes() and moved[k].tobytes() != before[k].tobytes(), k
        # the field and the i.i.d. model on a context that holds a trajectory
        rh.set_particle_trajectory(_arc_with_a_far_pose().compose(rig, cam.exposure))
        for model in ('iid', 'field'):
            fs, fgrid, fcdf = particles.sim_frames(opt, 25, 1, seed=9, model=model)
            fs = np.concatenate([fs, fs])
            fs['draw_seed'] = [3, 4]
            fwant = particles.expected_records(fs, fgrid, fcdf, sc.db, model=model, cam_hz=hz)
            rh.set_particle_tables(fgrid, fcdf)
            rh.set_particle_model(model, hz)
            got, cnt = rh.generate_drops(fs, H, W)
            for k in range(2):
                assert int(cnt[k]) == len(fwant[k]) and got[k].tobytes() == fwant[k].tobytes(), (model, k)
    finally:
        rh.close()


def _slots_of_records(s, dgrid, cdf, sc, hz, rig, view, traj):
    """The slot of every record expected_records makes for record s of view `view`: the kept rows of the loader's table."""
    table, m, W, H = particles._loaded_table(s, dgrid, cdf, sc.db, 'kitti', 'rig', hz, rig, view, trajectory=traj)
    keep = h.hb.filter_streaks(table, W, H)
    return np.asarray(table.pid)[keep]


def test_counter_draws_and_jitter_are_coherent(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    hz = opt['cam_hz']
    W, H = opt["cam_CCD_WH"]
    rig = cases.KITTI_STEREO
    traj = trajmod.Trajectory(np.array(cases.arc_poses(9)), 10.0)
    JIT = 3.0
    sims1, dgrid, cdf = particles.sim_frames(opt, 25, 1, seed=21, model='rig', rig=rig, trajectory=traj)
    sims = particles.rig_run_sims(sims1, [4, 5], 2)
    kw = dict(model='rig', cam_hz=hz, rig=rig, trajectory=traj, draws='counter')
    want = particles.expected_records(sims, dgrid, cdf, sc.db, jitter=JIT, **kw)
    straight = particles.expected_records(sims, dgrid, cdf, sc.db, **kw)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        cases.set_trajectory(rh, rig, traj, opt, hz)
        rh.set_particle_draws('counter')
        rh.set_particle_jitter(JIT)
        got, cnt = rh.generate_drops(sims, H, W)
        rh.set_particle_jitter(0.0)
        got0, _ = rh.generate_drops(sims, H, W)
    finally:
        rh.close()
    for k in range(4):
        assert int(cnt[k]) == len(want[k]) > 100
        cases.same_bytes(got[k], want[k], 'counter draws + jitter, frame %d' % k)
        cases.same_bytes(got0[k], straight[k], 'counter draws, frame %d' % k)
    cam = particles._traj_cam(particles.FrameCamera(opt, 0))
    seed = int(sims[0]['key0']) | (int(sims[0]['key1']) << 32)
    ids, lives = [], []
    for k in range(4):
        pid = _slots_of_records(sims[k], dgrid, cdf, sc, hz, rig, k % 2, traj)
        st = particles.rig_state(cam, dgrid, cdf[0], int(sims[k]['n_particles']), int(sims[k]['frame']), seed, hz, traj.box(rig, cam))
        assert len(pid) == len(got[k])
        ids.append(pid)
        lives.append(st['life'][pid])

    def tilt(k):          # the angle the jitter turned a non-Big record by: from its rotation terms before and after
        c0, s0, c, s = got0[k]['rot_cos'], got0[k]['rot_sin'], got[k]['rot_cos'], got[k]['rot_sin']
        return np.arctan2(s0 * c - c0 * s, c0 * c + s0 * s)

    pairs = 0
    for a, b in ((0, 1), (0, 2), (1, 3)):                     # two views of instant 4; view 0 and view 1 in frames 4 and 5
        _, ia, ib = np.intersect1d(ids[a], ids[b], return_indices=True)
        ok = lives[a][ia] == lives[b][ib]
        ia, ib = ia[ok], ib[ok]
        assert np.array_equal(got[a]['tex_index'][ia] % 10, got[b]['tex_index'][ib] % 10)
        thin = (got[a]['type'][ia] != 0) & (got[b]['type'][ib] != 0)
        ta, tb = tilt(a)[ia][thin], tilt(b)[ib][thin]
        assert np.all(np.abs(ta - tb) <= 1e-12) and np.abs(ta).max() > 1e-3       # (angle sums of unit vectors: a few roundings)
        pairs += int(thin.sum())
        print('frames %d, %d: %d slots in both, %d non-Big' % (a, b, len(ia), int(thin.sum())))
    assert pairs >= 100


def test_driver_runs_per_view_and_the_augmenter_agree(tmp_path, built, monkeypatch):
    """Two KITTI-sized frames: `main.py --particle_model rig --rig stereo:0.54 --rig_view v --trajectory poses.txt` for v = 0, 1;
    RainAugment(trajectory=) on the [B = 2, V = 2] clip (uint8) gives the RGB bytes of both runs' files; the run differs from the
    run without a trajectory; a trajectory with too few rows ends the run before any GPU work."""
    tmp = str(tmp_path)
    H, W, n = 375, 1242, 2
    src = os.path.join(tmp, 'source')
    h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), n, H, W, depth_m=None)
    streaks_db = os.path.join(tmp, 'rainstreakdb')
    h.synthetic.write_streak_db(streaks_db)
    poses = os.path.join(tmp, 'poses.txt')
    a = np.deg2rad(2.0)
    with open(poses, 'w') as fh:                                # KITTI axes: forward is +z; a left bend, a metre per frame
        for k in range(3):
            c, s = np.cos(k * a), np.sin(k * a)
            P = np.array([[c, 0.0, -s, -0.02 * k * k], [0.0, 1.0, 0.0, 0.0], [s, 0.0, c, 1.0 * k]])
            fh.write(' '.join('%.9e' % x for x in P.reshape(-1)) + '\n')
    short = os.path.join(tmp, 'short.txt')
    with open(short, 'w') as fh:
        fh.write('1 0 0 0 0 1 0 0 0 0 1 0\n')
    main = importlib.import_module('rain-rendering_amd.main')
    common = ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', streaks_db, '-i', '25', '--noverbose',
              '--device_particles', '--particle_model', 'rig', '--rig', 'stereo:0.54']
    for v in (0, 1):
        gen = main.main(common + ['--rig_view', str(v), '--trajectory', poses, '--output', os.path.join(tmp, 'view%d' % v)])
        assert len(gen.stats) == n and all(s['drops'] > 100 for s in gen.stats)
    main.main(common + ['--rig_view', '0', '--output', os.path.join(tmp, 'plain0')])
    with pytest.raises(ValueError, match='holds 1 poses'):
        main.main(common + ['--trajectory', short, '--output', os.path.join(tmp, 'outx')])
    with pytest.raises(SystemExit, match='--trajectory needs'):
        main.main(common[:-4] + ['--particle_model', 'field', '--trajectory', poses, '--output', os.path.join(tmp, 'outy')])
    sub = os.path.join('kitti', 'data_object', 'training', 'rain', '25mm')
    names = ['%06d.png' % i for i in range(n)]
    for f in names:
        assert open(os.path.join(tmp, 'view0', sub, 'rainy_image', f), 'rb').read() != open(os.path.join(tmp, 'plain0', sub, 'rainy_image', f), 'rb').read()
    img_dir = os.path.join(src, 'kitti', 'data_object', 'training', 'image_2')
    rgb = np.stack([np.array(Image.open(os.path.join(img_dir, f)).convert('RGB')) for f in names])
    depth = np.stack([np.array(Image.open(os.path.join(img_dir, 'depth', f))).astype(np.float32) / 256. for f in names])
    files = np.stack([np.stack([np.array(Image.open(os.path.join(tmp, 'view%d' % v, sub, 'rainy_image', f)))[..., :3] for v in (0, 1)])
                      for f in names])                                  # [n, V, H, W, 3]
    traj = trajmod.Trajectory.from_file(poses, hz=10.0)
    kw = dict(streaks_db=streaks_db, sequence='data_object/training', particle_model='rig', rig=cases.KITTI_STEREO)
    with pytest.raises(ValueError, match="needs particle_model='rig'"):
        augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', particle_model='field', trajectory=traj)
    aug = augment.RainAugment('kitti', trajectory=traj, **kw)
    try:
        img8 = torch.from_numpy(rgb.transpose(0, 3, 1, 2).copy()).to(DEV)
        dep = torch.from_numpy(depth).to(DEV)
        both = torch.stack([img8, img8], dim=1)                         # the synthetic set has one camera: both views start from its images
        dep2 = torch.stack([dep, dep], dim=1)
        rainy, mask = aug(both, dep2, 25, np.arange(n))
        assert tuple(rainy.shape) == (n, 2, 3, H, W) and tuple(mask.shape) == (n, 2, 1, H, W)
        assert np.array_equal(rainy.cpu().numpy().transpose(0, 1, 3, 4, 2), files)
        with pytest.raises(ValueError, match='outside the trajectory'):
            aug(both, dep2, 25, [0, 3])
        aug.set_trajectory(None)                                        # the rig stands still: the plain rig run's frames
        r0, _ = aug(both[:1], dep2[:1], 25, [0])
        plain = np.array(Image.open(os.path.join(tmp, 'plain0', sub, 'rainy_image', names[0])))[..., :3]
        assert np.array_equal(r0[0, 0].cpu().numpy().transpose(1, 2, 0), plain)
        aug.set_trajectory(traj)
        r1, _ = aug(both[1:], dep2[1:], 25, [1])                        # and back: random access
        assert torch.equal(r1, rainy[1:])
    finally:
        aug.close()


def test_invalid_arguments_are_refused(tmp_path, built):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    rig = cases.KITTI_STEREO
    cam = particles._traj_cam(particles.FrameCamera(opt, 0))
    traj = trajmod.Trajectory(np.array(cases.arc_poses(4)), 10.0)
    po = np.array(traj.compose(rig, cam.exposure))
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1, model='rig', rig=rig, trajectory=traj)
    rh = cases.rain_hip(sc)
    try:
        rh.set_particle_tables(dgrid, cdf)
        with pytest.raises(RuntimeError, match='no rig set'):
            rh.set_particle_trajectory(po)
        rh.set_particle_rig(rig.as_records(), traj.box(rig, cam))
        rh.set_particle_model('rig', 10.0)
        for bad in ([0, 1, 1, 2], [0, 2, 1, 3]):
            with pytest.raises(RuntimeError, match='strictly ascending'):
                rh.set_particle_trajectory(po, frame=bad)
        b = po.copy(); b['R1'][2, 1, 0] = 1.0 + 1e-6
        with pytest.raises(RuntimeError, match='instant 2, view 1, end of the exposure.*orthonormal'):
            rh.set_particle_trajectory(b)
        b = po.copy(); b['R0'][1, 0, 8] = -b['R0'][1, 0, 8]; b['R0'][1, 0, 6] = -b['R0'][1, 0, 6]; b['R0'][1, 0, 7] = -b['R0'][1, 0, 7]
        with pytest.raises(RuntimeError, match='instant 1, view 0, start of the exposure.*orthonormal'):
            rh.set_particle_trajectory(b)                               # a reflection: determinant -1
        b = po.copy(); b['c1'][3, 0, 1] = np.nan
        with pytest.raises(RuntimeError, match='instant 3, view 0, end of the exposure.*finite'):
            rh.set_particle_trajectory(b)
        b = po.copy(); b['R0'][0, 1, 4] = np.inf
        with pytest.raises(RuntimeError, match='instant 0, view 1, start of the exposure.*finite'):
            rh.set_particle_trajectory(b)
        b = po.copy(); b['c0'][0, 0] = (8e5, 0.0, 8e5)
        with pytest.raises(RuntimeError, match='beyond 1e6 m'):
            rh.set_particle_trajectory(b)
        lib = h.hb.load_library()
        assert lib.rr_set_particle_trajectory(rh.h, (1 << 20) + 1, None, None) == -1 and b'2^20' in lib.rr_last_error(rh.h)
        assert lib.rr_set_particle_trajectory(rh.h, -1, None, None) == -1 and b'2^20' in lib.rr_last_error(rh.h)
        # when generating: an instant whose time index the table does not hold
        rh.set_particle_trajectory(po[[0, 1, 3]], frame=[0, 1, 3])
        got, cnt = rh.generate_drops(particles.rig_run_sims(sims, [3, 0], 2), 375, 1242)
        assert all(int(c) > 100 for c in cnt)
        with pytest.raises(RuntimeError, match=r'frame 2 \(instant 1\) is not in the trajectory'):
            rh.generate_drops(particles.rig_run_sims(sims, [1, 2], 2), 375, 1242)
        noisy = particles.rig_run_sims(sims, [0], 2)
        noisy['run_pos'] = 1
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.generate_drops(noisy, 375, 1242)
        with pytest.raises(RuntimeError, match='angular noise'):
            rh.set_particle_noise(2.0, 1.0, [0], [0])
        # a rig with another number of views drops the table: the one-view rig runs as the plain rig model
        rh.set_particle_rig(cases.MONO.as_records(), cases.MONO.box(cam))
        got, cnt = rh.generate_drops(particles.rig_run_sims(sims, [2], 1), 375, 1242)
        assert int(cnt[0]) > 100
    finally:
        rh.close()
