"""CPU tier: the RIG particle model (tools/particles.py make_rig_particles, rr_particles.h make_rig_slot / rig_view_particle,
rig.py) -- one persistent, stateless particle field in the rig's frame, seen by several cameras.

  1. the g++ build of the RR_HD statement (tests/hostemu/particles_emu.cpp: the code k_rig_particles runs) == numpy, bit for bit;
  2. cross-view geometry: a slot kept by two views at one instant is ONE point of the lattice world; stereo disparity;
  3. every view has the i.i.d. model's law (the thresholds and the control of tests/test_particle_field_host.py);
  4. motion: a slot kept at k and k + 1 in one life has moved by its velocity / cam_hz;
  5. random access: an instant alone, a subset or a permutation of the active views: the same bits per (instant, view);
  6. no double vision: with the host's r the nearest lattice image is the only one a view can see; 1 % less and another is;
  7. every refusal of the Python layer; 8. RainAugment.plan of a [B, V] clip."""
import importlib
import json
import os

import numpy as np
import pytest

import helpers as h
import particle_cases as cases
import particle_emu as pe

particles = importlib.import_module('rain-rendering_amd.tools.particles')
rigmod = importlib.import_module('rain-rendering_amd.rig')
db = importlib.import_module('rain-rendering_amd.common.db')
U = cases.U
CONFIGS, IDS = cases.CONFIGS, cases.IDS


@pytest.fixture(scope='module')
def emu(built):
    return pe.load()


# ---- 1. g++ == numpy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset,rs,rate,rig", CONFIGS, ids=IDS)
def test_gxx_build_equals_numpy(tmp_path, emu, dataset, rs, rate, rig):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options(dataset, sim_steps={"cam_motion": np.array([30.0])})
    hz = float(opt['cam_hz'])
    V = len(rig)
    sims, dgrid, cdf = particles.sim_frames(opt, rate, 1, render_scale=rs, seed=1234 + 2 ** 40, model='rig', rig=rig)
    sims = particles.rig_run_sims(sims, [0, 1, 2 ** 31 + 5], V)
    want = particles.expected_records(sims, dgrid, cdf, sc.db, model='rig', cam_hz=hz, rig=rig)
    cam = particles.FrameCamera(opt, 0)
    box = np.array(rig.box(cam), np.float64)
    views = rig.as_records()
    W, H = opt["cam_CCD_WH"][0] // rs, opt["cam_CCD_WH"][1] // rs
    ratio_db = np.ascontiguousarray(np.asarray(sc.db.ratio, np.float64)[:4])
    tab = np.ascontiguousarray(cdf[0])
    total = 0
    for i, s in enumerate(sims):
        v = i % V
        n = int(s['n_particles'])
        seed = int(s['key0']) | (int(s['key1']) << 32)
        rec, life = particles.make_rig_particles(cam, dgrid, tab, n, int(s['frame']), seed, hz, rig.views[v], box, cull=False)
        kept, _ = particles.make_rig_particles(cam, dgrid, tab, n, int(s['frame']), seed, hz, rig.views[v], box)
        run = pe.run(model='rig', sim=sims[i:i + 1], cam_hz=hz, view=views[v:v + 1], box=box, dgrid=dgrid, cdf=tab)
        out, ins, lf, _ = pe.all_slots(run)
        pe.assert_slots_equal(out, lf, rec, life, i)
        assert np.array_equal(np.nonzero(ins)[0], kept['pid']) and len(kept) > 100
        got, _ = pe.records(run, H, W, ratio_db)
        assert len(got) == len(want[i]) > 100
        pe.assert_records_equal(got, want[i], 'stream', i)        # the draws pick one of the block of ten
        total += len(got)
    print('%s rs %d %d mm/hr, %d views: %d records compared' % (dataset, rs, rate, V, total))
    assert want[0].tobytes() != want[V].tobytes()                 # the field moves from instant to instant


# ---- 2. cross-view geometry ------------------------------------------------------------------------------------------
def _period(cam, dgrid, cdf, slots, seed, box):
    D = particles.sample_diameter(dgrid, cdf, particles.unit32(particles.philox4x32(np.asarray(slots, np.uint64), 0, 0, 1, *particles._key(seed))[0]))
    z_max = np.minimum(((D * 1e-3) * cam.fpx) / 1.0, 15.0)
    return 2.0 * (box[0] * z_max), 2.0 * (box[1] * z_max + box[2])


@pytest.mark.parametrize("dataset,rate,rig,n_inst", [('kitti', 25, cases.KITTI_STEREO, 2), ('nuscenes', 100, cases.RING6, 2)], ids=['stereo', 'ring6'])
def test_two_views_see_one_world(dataset, rate, rig, n_inst):
    """Every slot kept by two views at one instant: R_a^T p_a + c_a and R_b^T p_b + c_b agree modulo the lattice period 2 b(D) in
    x and z and without any period in y, within _world_bound.  Stereo, pairs on the same lattice image: ip1.x differs by
    fpx baseline / depth.  (Slots nearer than 5 cm are left out: their depth is clamped for the projection.)"""
    opt = cases.options(dataset, sim_steps={"cam_motion": np.array([50.0])})
    cam = particles.FrameCamera(opt, 0)
    box = rig.box(cam)
    _, dgrid, cdf, _ = particles.rig_expected_count(cam, rate, box)
    shared = same_image = 0
    for k in range(n_inst):
        recs = [particles.rig_frame(opt, rate, 7 + k, rig, v, seed=21)[0] for v in range(len(rig))]
        for a in range(len(rig)):
            for b in range(a + 1, len(rig)):
                _, ia, ib = np.intersect1d(recs[a]['pid'], recs[b]['pid'], return_indices=True)
                free = (recs[a]['wp1'][ia, 2] < -0.05) & (recs[b]['wp1'][ib, 2] < -0.05)
                ra, rb = recs[a][ia[free]], recs[b][ib[free]]
                if len(ra) == 0:
                    continue
                w, _ = _period(cam, dgrid, cdf, ra['pid'], 21, box)
                r = cases._world(ra, rig.views[a]) - cases._world(rb, rig.views[b])
                m = np.rint(r[:, [0, 2]] / w[:, None])
                r[:, 0] -= m[:, 0] * w
                r[:, 2] -= m[:, 1] * w
                bound = cases._world_bound(ra, rig.views[a], w) + cases._world_bound(rb, rig.views[b], w) + 2.0 * U * w * (1.0 + np.abs(m).max(axis=1))
                print('instant %d views %d, %d: %d shared slots, worst |residual| / bound %.3f, %d on another lattice image'
                      % (7 + k, a, b, len(ra), (np.abs(r).max(axis=1) / bound).max(), int((m != 0).any(axis=1).sum())))
                assert np.all(np.abs(r) <= bound[:, None]), (np.abs(r).max(axis=1) / bound).max()
                shared += len(ra)
                if rig is cases.KITTI_STEREO:
                    base = rig.views[b][1][0] - rig.views[a][1][0]
                    on = ~(m != 0).any(axis=1)
                    depth = -ra['wp1'][on, 2]
                    assert np.array_equal(depth, -rb['wp1'][on, 2])      # parallel cameras at one z: the same operations
                    xa, xb = ra['wp1'][on, 0], rb['wp1'][on, 0]
                    want = (cam.fpx * base) / depth
                    got = ra['ip1'][on, 0] - rb['ip1'][on, 0]
                    # x_c = (X - c_x) - floor(.) w: three roundings of values <= |x_c| + w + |c_x| per view; ip = W / 2 + fpx x_c / depth:
                    # the error of x_c times fpx / depth, two roundings of the quotient's size, one of the sum's; then the test's
                    # difference and its own fpx base / depth (two roundings)
                    ex = sum(3.0 * U * (np.abs(x) + w[on] + abs(base)) for x in (xa, xb))
                    e_ip = sum(2.0 * U * np.abs(cam.fpx * x / depth) + U * np.abs(ip) for x, ip in ((xa, ra['ip1'][on, 0]), (xb, rb['ip1'][on, 0])))
                    tol = (cam.fpx / depth) * ex + e_ip + U * np.abs(got) + 2.0 * U * np.abs(want)
                    print('  disparity: %d pairs, worst |error| / bound %.3f, disparities %.2f .. %.1f px'
                          % (on.sum(), (np.abs(got - want) / tol).max(), want.min(), want.max()))
                    assert np.all(np.abs(got - want) <= tol)
                    same_image += int(on.sum())
    print('%d shared slots compared' % shared)
    assert shared >= 200
    if rig is cases.KITTI_STEREO:
        assert same_image >= 200


# ---- 3. the law of every view ------------------------------------------------------------------------------------------
def _rig_sample(rig, view, seed0):
    """cases._sample for one view of a rig: cases.N_LAW frames of KITTI at 25 mm/hr, each under a seed of its own."""
    opt = cases.options('kitti')
    cam = particles.FrameCamera(opt, 0)
    counts, D, depth, px, py = [], [], [], [], []
    for i in range(cases.N_LAW):
        rec, _ = particles.rig_frame(opt, 25, 7 * i + 3, rig, view, seed=seed0 + i)
        counts.append(len(rec))
        D.append(rec['wd1'] * 1e3)
        depth.append(-rec['wp1'][:, 2])
        px.append(rec['ip1'][:, 0])
        py.append(rec['ip1'][:, 1])
    return dict(cam=cam, counts=np.array(counts), D=np.concatenate(D), depth=np.concatenate(depth), px=np.concatenate(px), py=np.concatenate(py))


def test_every_view_has_the_iid_models_law():
    """Each view of the stereo rig and of a ring with pitched cameras against the i.i.d. model: the count within four Poisson
    standard errors, Kolmogorov-Smirnov on diameter, depth and image position -- cases._same_law with tf's thresholds and its
    i.i.d.-against-itself control."""
    iid_a, iid_b = cases._sample('iid', 1000), cases._sample('iid', 5000)
    control = cases._same_law(iid_a, iid_b)
    assert all(v < 1 for v in control.values()), control
    mean = particles.expected_count(iid_a['cam'], 25)[0]
    for name, rig in (('stereo', cases.KITTI_STEREO), ('pitched ring', cases.PITCHED)):
        for v in range(len(rig)):
            s = _rig_sample(rig, v, 9000 + 1000 * v)
            got, got_b = cases._same_law(s, iid_a), cases._same_law(s, iid_b)
            print('%s view %d: mean count %.1f (model %.1f); statistic / threshold vs iid: %s; vs iid (other seeds): %s'
                  % (name, v, s['counts'].mean(), mean, got, got_b))
            assert abs(s['counts'].mean() - mean) < 4 * np.sqrt(mean / cases.N_LAW)
            assert all(x < 1 for x in got.values()), (name, v, got)
            assert all(x < 1 for x in got_b.values()), (name, v, got_b)


# ---- 4. motion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,dataset,rate", [(cases.KITTI_STEREO, 'kitti', 25), (cases.PITCHED, 'kitti', 25)], ids=['stereo', 'pitched-ring'])
def test_tracks_move_by_velocity_over_cam_hz(rig, dataset, rate):
    """A slot kept by view v at k and k + 1 in one life: p(k + 1) - p(k) = R_v velocity / cam_hz up to whole lattice periods --
    checked on the residual turned back into the rig frame, within the rounding of the two positions (_world_bound), of the
    rig-frame state (cases._track_bounds with the rig's box) and of the expected displacement."""
    opt = cases.options(dataset, sim_steps={"cam_motion": np.array([50.0])})
    cam = particles.FrameCamera(opt, 0)
    box = rig.box(cam)
    _, dgrid, cdf, _ = particles.rig_expected_count(cam, rate, box)
    n_slots = int(particles.rig_slot_counts(opt, rate, 1, rig, seed=11)[0])
    dt = 1.0 / cam.hz
    total = 0
    for k in list(range(0, 16)) + list(range(1000, 1016)):      # (at 10 frames a second few drops are seen twice: many instants)
        st = particles.rig_state(cam, dgrid, cdf, n_slots, k, 11, cam.hz, box)
        for v in range(len(rig)):
            ra, la = particles.rig_frame(opt, rate, k, rig, v, seed=11)
            rb, lb = particles.rig_frame(opt, rate, k + 1, rig, v, seed=11)
            _, ia, ib = np.intersect1d(ra['pid'], rb['pid'], return_indices=True)
            ok = (la[ia] == lb[ib]) & (ra['wp1'][ia, 2] < -0.05) & (rb['wp1'][ib, 2] < -0.05)
            ra, rb, life = ra[ia[ok]], rb[ib[ok]], la[ia[ok]]
            if len(ra) == 0:
                continue
            vel = st['vel'][ra['pid']]
            w, wy = 2.0 * st['b'][ra['pid']], 2.0 * st['by'][ra['pid']]
            r = (cases._world(rb, rig.views[v]) - cases._world(ra, rig.views[v])) - vel * dt
            m = np.rint(r[:, [0, 2]] / w[:, None])
            r[:, 0] -= m[:, 0] * w
            r[:, 2] -= m[:, 1] * w
            bound = cases._state_bounds(vel, w, wy, life, dt) + (cases._world_bound(ra, rig.views[v], w) + cases._world_bound(rb, rig.views[v], w))[:, None]
            print('view %d, %d -> %d: %d kept again, worst |residual| / bound per axis %s' % (v, k, k + 1, len(ra), (np.abs(r) / bound).max(axis=0)))
            assert np.all(np.abs(r) <= bound), (np.abs(r) / bound).max(axis=0)
            total += len(ra)
    print('%d tracks compared' % total)
    assert total >= 100


# ---- 5. random access ------------------------------------------------------------------------------------------------
def test_an_instant_and_a_view_alone_have_the_runs_bits(tmp_path):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    hz = opt['cam_hz']
    rig = cases.KITTI_STEREO
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1, seed=3, model='rig', rig=rig)
    run = particles.rig_run_sims(sims, np.arange(6), 2)
    kw = dict(model='rig', cam_hz=hz, rig=rig)
    whole = particles.expected_records(run, dgrid, cdf, sc.db, **kw)                       # frame 2 k + v
    alone = particles.expected_records(run[10:12], dgrid, cdf, sc.db, **kw)                # instant 5
    assert len(whole[10]) > 100 and whole[10].tobytes() == alone[0].tobytes() and whole[11].tobytes() == alone[1].tobytes()
    only1 = particles.expected_records(run[1::2], dgrid, cdf, sc.db, view=[1], **kw)       # active = [1]
    assert all(only1[k].tobytes() == whole[2 * k + 1].tobytes() for k in range(6))
    assert particles.expected_records(run[1::2], dgrid, cdf, sc.db, view=1, **kw)[3].tobytes() == whole[7].tobytes()
    swapped = particles.expected_records(run, dgrid, cdf, sc.db, view=[1, 0], **kw)        # a permuted active list permutes the tables
    assert all(swapped[2 * k].tobytes() == whole[2 * k + 1].tobytes() and swapped[2 * k + 1].tobytes() == whole[2 * k].tobytes() for k in range(6))
    assert whole[10].tobytes() != whole[11].tobytes() and whole[8].tobytes() != whole[10].tobytes()
    for k in range(12):
        assert np.all(np.diff(particles.rig_frame(opt, 25, k // 2, rig, k % 2, seed=3)[0]['pid']) > 0)   # ascending slots, none twice
    with pytest.raises(ValueError, match='multiple'):
        particles.expected_records(run[:3], dgrid, cdf, sc.db, **kw)


# ---- 6. no double vision -----------------------------------------------------------------------------------------------
def test_the_nearest_image_is_the_only_visible_one():
    """With the host's r (Rig.box) a view's frustum lies inside the lattice cell centred on its camera: no lattice image other than
    the nearest one passes the view's cull, so no view sees a particle twice and the cull by the nearest image misses none.
    With r 1 % smaller a far corner of the frustum of the view that attains r sticks out of the cell: an image other than the
    nearest is visible there -- in the periodic world that slot would be seen by an image the statement does not look at.
    (A realistic camera cannot see two images of one slot at once: its frustum is narrower than a period in every direction;
    what a too small r breaks is the nearest-image cull, and that is what is shown.)"""
    opt = cases.options('nuscenes')
    cam = particles.FrameCamera(opt, 0)
    rig = cases.RING6
    box = rig.box(cam)
    _, dgrid, cdf, _ = particles.rig_expected_count(cam, 100, box)
    n = 400000
    others = [(ix, iz) for ix in (-1, 0, 1) for iz in (-1, 0, 1) if (ix, iz) != (0, 0)]
    tight = (0.99 * box[0], box[1], box[2])
    seen_tight = 0
    for v in range(len(rig)):
        near, _ = particles.make_rig_particles(cam, dgrid, cdf, n, 4, 77, cam.hz, rig.views[v], box)
        assert len(np.unique(near['pid'])) == len(near) > 1000
        for img in others:
            far, _ = particles.make_rig_particles(cam, dgrid, cdf, n, 4, 77, cam.hz, rig.views[v], box, image=img)
            assert len(far) == 0, (v, img, len(far))
            seen_tight += len(particles.make_rig_particles(cam, dgrid, cdf, n, 4, 77, cam.hz, rig.views[v], tight, image=img)[0])
    print('%d slots visible through an image other than the nearest with r 1 %% too small' % seen_tight)
    assert seen_tight > 0


# ---- 7. arguments --------------------------------------------------------------------------------------------------------
def test_refusals_of_the_python_layer(tmp_path):
    augment = importlib.import_module('rain-rendering_amd.augment')
    eye = np.eye(3)
    with pytest.raises(ValueError, match='1 to 8 views'):
        rigmod.Rig([])
    with pytest.raises(ValueError, match='1 to 8 views'):
        rigmod.Rig([(eye, [0, 0, 0])] * 9)
    with pytest.raises(ValueError, match='orthonormal'):
        rigmod.Rig([(eye * 1.001, [0, 0, 0])])
    with pytest.raises(ValueError, match='orthonormal'):
        rigmod.Rig([(np.diag([1.0, 1.0, -1.0]), [0, 0, 0])])                 # a reflection: determinant -1
    with pytest.raises(ValueError, match='finite'):
        rigmod.Rig([(eye, [0, np.nan, 0])])
    with pytest.raises(ValueError, match='baseline'):
        rigmod.Rig.stereo(0.0)
    with pytest.raises(ValueError, match='pitches'):
        rigmod.Rig.yaw_ring([0, 90], 1.0, pitches_deg=[0])
    spec = os.path.join(str(tmp_path), 'rig.json')
    with open(spec, 'w') as fh:
        json.dump({"views": [{"R": eye.reshape(9).tolist(), "c": [0, 0, 0], "fpx": 700.0}]}, fh)
    with pytest.raises(ValueError, match='intrinsics'):
        rigmod.Rig.from_spec(spec)                                           # per-view intrinsics are out of scope
    with open(spec, 'w') as fh:
        json.dump({"views": [{"R": v[0].reshape(9).tolist(), "c": v[1].tolist()} for v in cases.RING6.views]}, fh)
    assert rigmod.Rig.from_spec(spec).as_records().tobytes() == cases.RING6.as_records().tobytes()
    assert rigmod.Rig.from_spec('stereo:0.54').as_records().tobytes() == cases.KITTI_STEREO.as_records().tobytes()
    for bad in ([], [0, 0], [2], [-1], [0.5]):
        with pytest.raises(ValueError, match='distinct'):
            rigmod.check_active(bad, 2)
    opt = cases.options('kitti')
    with pytest.raises(ValueError, match='rig='):
        particles.sim_frames(opt, 25, 1, model='rig')
    with pytest.raises(ValueError, match='one camera'):
        particles.sim_frames(cases.options('kitti', sim_mode='steps', sim_steps={"cam_focal": np.array([4.0, 6.0])}), 25, 2, model='rig', rig=cases.KITTI_STEREO)
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1, model='rig', rig=cases.KITTI_STEREO)
    with pytest.raises(ValueError, match='angular noise'):
        particles.expected_records(sims, dgrid, cdf, None, model='rig', cam_hz=10.0, rig=cases.KITTI_STEREO, noise_std=2.0, noise_scale=1.0)
    # RainAugment
    root = str(tmp_path)
    h.synthetic.write_streak_db(os.path.join(root, 'rainstreakdb'))
    kw = dict(streaks_db=os.path.join(root, 'rainstreakdb'), sequence='data_object/training')
    with pytest.raises(ValueError, match='go together'):
        augment.RainAugment('kitti', particle_model='rig', **kw)
    with pytest.raises(ValueError, match='go together'):
        augment.RainAugment('kitti', particle_model='field', rig=cases.KITTI_STEREO, **kw)
    with pytest.raises(ValueError, match='views='):
        augment.RainAugment('kitti', views=[0], **kw)
    with pytest.raises(TypeError, match='rig.Rig'):
        augment.RainAugment('kitti', particle_model='rig', rig=[(eye, [0, 0, 0])], **kw)
    with pytest.raises(ValueError, match='distinct'):
        augment.RainAugment('kitti', particle_model='rig', rig=cases.KITTI_STEREO, views=[0, 2], **kw)
    aug = augment.RainAugment('kitti', particle_model='rig', rig=cases.KITTI_STEREO, **kw)
    import torch
    H, W = aug.frame_size()
    with pytest.raises(ValueError, match=r'\[B, V = 2, 3, H, W\]'):
        aug._validate(torch.zeros((2, 3, H, W), dtype=torch.uint8), torch.zeros((2, H, W)))
    with pytest.raises(ValueError, match=r'\[B, V = 2, 3, H, W\]'):
        aug._validate(torch.zeros((2, 1, 3, H, W), dtype=torch.uint8), torch.zeros((2, 1, H, W)))
    with pytest.raises(ValueError, match='depth'):
        aug._validate(torch.zeros((2, 2, 3, 8, 8), dtype=torch.uint8), torch.zeros((2, 8, 8)))
    assert aug._validate(torch.zeros((2, 2, 3, 8, 8), dtype=torch.uint8), torch.zeros((2, 2, 1, 8, 8))) == (2, 8, 8)
    with pytest.raises(ValueError, match='2 values for a batch of 3'):
        aug.plan(25, [0, 1], B=3)                                           # one frame index per instant, not per image


# ---- 8. RainAugment.plan -----------------------------------------------------------------------------------------------
def test_augment_plan_of_a_rig_clip(tmp_path):
    augment = importlib.import_module('rain-rendering_amd.augment')
    SEQ = 'data_object/training'
    root = str(tmp_path)
    h.synthetic.write_streak_db(os.path.join(root, 'rainstreakdb'))
    kw = dict(streaks_db=os.path.join(root, 'rainstreakdb'), sequence=SEQ, particle_model='rig', rig=cases.KITTI_STEREO)
    aug = augment.RainAugment('kitti', **kw)
    right = augment.RainAugment('kitti', views=[1], **kw)
    st = db.settings('kitti')
    opts = db.sim('kitti', SEQ, os.path.join('particles', 'kitti'))['options']
    n_sim = particles.n_sim_frames(opts)
    sims, dgrid, cdf = particles.sim_frames(opts, 25, n_sim, render_scale=st['render_scale'], seed=0, model='rig', rig=cases.KITTI_STEREO)
    idx = n_sim - 2 + np.arange(5)                                # a clip across the end of the simulated frames: time goes on
    p = aug.plan(25, idx)
    assert p['particle_model'] == 'rig' and p['cam_hz'] == float(opts['cam_hz']) and p['views'] == [0, 1]
    want = particles.rig_run_sims(sims, idx, 2)
    assert p['sims'].tobytes() == want.tobytes() and len(p['sims']) == 10 and p['fog'].shape == (10, 4)
    assert np.array_equal(p['sims']['frame'], np.repeat(idx, 2)) and np.array_equal(p['sims']['draw_seed'], np.repeat(idx, 2))
    assert np.array_equal(p['d_grid'], dgrid) and np.array_equal(p['cdf'], np.atleast_2d(cdf))
    assert p['rig_views'].tobytes() == cases.KITTI_STEREO.as_records().tobytes()
    assert tuple(p['rig_box']) == tuple(cases.KITTI_STEREO.box(particles.FrameCamera(opts, 0)))
    n_slots = int(p['sims']['n_particles'][0])
    assert set(p['sims']['n_particles'].tolist()) == {n_slots}
    assert p['drops_cap'] == (min(max(1024, n_slots), 2 ** 16) + 3) // 4 * 4
    q = right.plan(25, idx)
    assert q['views'] == [1] and q['sims'].tobytes() == want[1::2].tobytes() and q['fog'].shape == (5, 4)
