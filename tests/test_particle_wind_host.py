"""CPU tier: the mean wind of the particle generators (tools/particles.py wind=, rr_particles.h WIND, rr_set_particle_wind) -- the air's
mean horizontal velocity (wx, wz) joins every drop's own: vx = wind_life + wx, vz = speed + wz.

  1. the g++ build of the RR_HD statement (tests/hostemu/particles_emu.cpp: the code the WIND kernels run) == numpy, bit for bit: i.i.d.,
     field, rig (stereo, a yaw ring) and a rig under a trajectory yawed 37 degrees and pitched; three winds, both draws, jitter 0 / 5;
  2. wind=(0, 0) gives the bytes of the functions called without the keyword, for every model;
  3. kinematics: a slot seen again in its life has moved by (vx, -v, vz) / cam_hz; every kept record's streak is (vx, -v, vz) exposure
     in the view's axes;
  4. the law: a field frame under (6, -2) follows the i.i.d. model's law (tests/test_particle_field_host.py's test and thresholds);
  5. slant: with no scatter and no ego-motion every streak leans the wind's way, by wx / v(D); a view yawed 180 degrees sees the
     opposite; under a trajectory the wind is a world vector;
  8. every refusal of the Python layer and of the driver's argument handling; RainAugment.plan carries the wind."""
import importlib
import os

import numpy as np
import pytest

import helpers as h
import particle_cases as cases
import particle_emu as pe

particles = importlib.import_module('rain-rendering_amd.tools.particles')
trajmod = importlib.import_module('rain-rendering_amd.trajectory')
U = cases.U
SEED = cases.SEED
WINDS = [(3.0, 0.0), (-7.5, 2.0), (0.0, -4.0)]
CASES = cases.CASES                                       # (name, model, rig, trajectory): what items 1 and 2 cover
CASE_IDS = [c[0] for c in CASES]


@pytest.fixture(scope='module')
def emu(built):
    return pe.load()


@pytest.fixture(scope='module')
def sdb(tmp_path_factory):
    return h.Scene(tmp_path_factory.mktemp('wind'), 64, 96, 10).db     # (only the texture ratios are used)


def _all_particles(model, cam, dgrid, tab, s, hz, rig, traj, view, box, wind=None):
    """Every particle / slot of record `s` (cull off): (records, life) of the numpy statement; wind=None: without the keyword."""
    n, k = int(s['n_particles']), int(s['frame'])
    seed = int(s['key0']) | (int(s['key1']) << 32)
    kw = {} if wind is None else dict(wind=wind)
    if model == 'iid':
        rec = particles.make_particles(cam, dgrid, tab, n, k, seed, **kw)
        return rec, np.zeros(n)
    if model == 'field':
        return particles.make_field_particles(cam, dgrid, tab, n, k, seed, hz, cull=False, **kw)
    if traj is None:
        return particles.make_rig_particles(cam, dgrid, tab, n, k, seed, hz, rig.views[view], tuple(box), cull=False, **kw)
    po = traj.compose(rig, cam.exposure)[k, view]
    return particles.make_rig_particles(cam, dgrid, tab, n, k, seed, hz, (po['R0'], po['c0']), tuple(box), cull=False,
                                        view_end=(po['R1'], po['c1']), **kw)


# ---- 1. g++ == numpy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,rig,traj", CASES, ids=CASE_IDS)
def test_gxx_build_equals_numpy(emu, sdb, name, model, rig, traj):
    frames = [0, 1] if traj is not None else [3, 2 ** 31 + 5]
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, frames)
    hz = float(opt['cam_hz'])
    V = len(rig) if rig is not None else 1
    W, H = opt["cam_CCD_WH"]
    ratio_db = np.ascontiguousarray(np.asarray(sdb.ratio, np.float64)[:4])
    tab = np.ascontiguousarray(cdf[0])
    views = rig.as_records() if rig is not None else None
    poses = traj.compose(rig, cam.exposure) if traj is not None else None
    plain = particles.expected_records(sims, dgrid, cdf, sdb, **kw)
    total = 0
    for wind in WINDS:
        want = {(d, j): particles.expected_records(sims, dgrid, cdf, sdb, draws=d, jitter=j, wind=wind, **kw)
                for d in ('counter', 'stream') for j in (0.0, 5.0)}
        for i, s in enumerate(sims):
            v = i % V
            view = views[v:v + 1] if views is not None and traj is None else None
            po = poses[int(s['frame']), v:v + 1] if traj is not None else None
            air = dict(model=model, sim=sims[i:i + 1], cam_hz=hz, view=view, pose=po, box=box, dgrid=dgrid, cdf=tab, wind=wind)
            # every particle / slot, kept or not
            rec, life = _all_particles(model, cam, dgrid, tab, s, hz, rig, traj, v, box, wind)
            out, ins, lf, _ = pe.all_slots(pe.run(**air))
            pe.assert_slots_equal(out, lf, rec, life, (i, wind))
            # the finished records
            for (draws, jit), recs in want.items():
                got, _ = pe.records(pe.run(counter=draws == 'counter', jitter=jit, **air), H, W, ratio_db)
                m, w = len(got), recs[i]
                assert m == len(w) > 100, (i, wind, draws, jit, m, len(w))
                pe.assert_records_equal(got, w, draws, (i, wind, draws, jit), cases._same_field)
                total += m
            assert want[('stream', 0.0)][i].tobytes() != plain[i].tobytes()          # the wind does something
    print('%s: %d records compared' % (name, total))


# ---- 2. wind off == today ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,rig,traj", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("wind_sigma", [1.0, 0.0])
def test_zero_wind_gives_the_bytes_without_the_keyword(sdb, name, model, rig, traj, wind_sigma):
    """wind_sigma = 0 is the case an added zero would change: block_wind gives -0.0 for half of the drops."""
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, [0, 1])
    sims['wind_sigma'] = wind_sigma
    hz = float(opt['cam_hz'])
    for draws, jit in (('stream', 0.0), ('counter', 5.0)):
        a = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, **kw)
        b = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, wind=(0.0, 0.0), **kw)
        c = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, wind=(-0.0, 0), **kw)
        assert all(len(x) > 100 and x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(a, b, c))
    V = len(rig) if rig is not None else 1
    tab = np.ascontiguousarray(cdf[0])
    n_neg = 0
    for i, s in enumerate(sims):
        ckw = dict(wind_sigma=wind_sigma)
        n, k = int(s['n_particles']), int(s['frame'])
        seed = int(s['key0']) | (int(s['key1']) << 32)
        if model == 'iid':
            pair = [(particles.make_particles(cam, dgrid, tab, n, k, seed, **ckw, **w),) for w in ({}, dict(wind=(0.0, 0.0)))]
        elif model == 'field':
            pair = [particles.make_field_particles(cam, dgrid, tab, n, k, seed, hz, cull=False, **ckw, **w) for w in ({}, dict(wind=(0.0, 0.0)))]
        else:
            po = traj.compose(rig, cam.exposure)[k, i % V] if traj is not None else None
            pose = rig.views[i % V] if po is None else (po['R0'], po['c0'])
            end = None if po is None else (po['R1'], po['c1'])
            pair = [particles.make_rig_particles(cam, dgrid, tab, n, k, seed, hz, pose, tuple(box), cull=False, view_end=end, **ckw, **w)
                    for w in ({}, dict(wind=(0.0, 0.0)))]
            st = [particles.rig_state(cam, dgrid, tab, n, k, seed, hz, tuple(box), **ckw, **w) for w in ({}, dict(wind=(0.0, 0.0)))]
            assert all(st[0][key].tobytes() == st[1][key].tobytes() for key in st[0])
            n_neg += int(np.signbit(st[0]['vel'][:, 0]).sum()) if wind_sigma == 0.0 else 0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(*pair))
    if model == 'rig' and wind_sigma == 0.0:
        assert n_neg > 0                                          # the -0.0 winds are there
    if model == 'field':
        opt2 = cases.options('kitti')
        a, b = particles.generate(opt2, 25, 2, seed=3, model='field'), particles.generate(opt2, 25, 2, seed=3, model='field', wind=(0, 0))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        fa, fb = particles.field_frame(opt2, 25, 4, seed=3), particles.field_frame(opt2, 25, 4, seed=3, wind=(0.0, 0.0))
        assert fa[0].tobytes() == fb[0].tobytes() and fa[1].tobytes() == fb[1].tobytes()
        ka = particles.field_kinematics(cam, dgrid, tab, fa[0]['pid'], fa[1], 3)
        kb = particles.field_kinematics(cam, dgrid, tab, fa[0]['pid'], fa[1], 3, wind=(0.0, 0.0))
        assert ka[0].tobytes() == kb[0].tobytes() and ka[1].tobytes() == kb[1].tobytes()
    if model == 'iid':
        opt2 = cases.options('kitti')
        a, b = particles.generate(opt2, 25, 2, seed=3), particles.generate(opt2, 25, 2, seed=3, wind=(0, 0))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    if model == 'rig':
        opt2 = cases.options('kitti')
        a = particles.rig_frame(opt2, 25, 1, rig, 0, seed=3, trajectory=traj)
        b = particles.rig_frame(opt2, 25, 1, rig, 0, seed=3, trajectory=traj, wind=(0.0, 0.0))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 3. kinematics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wind", [(6.0, -2.0), (-7.5, 2.0)])
def test_field_tracks_move_by_the_windy_velocity(wind):
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([50.0])})
    cam = particles.FrameCamera(opt, 0)
    _, dgrid, cdf, _ = particles.expected_count(cam, 25)
    dt = 1.0 / cam.hz
    total = 0
    for k in (0, 1, 2, 1000, 1001):
        ra, la = particles.field_frame(opt, 25, k, seed=11, wind=wind)
        rb, lb = particles.field_frame(opt, 25, k + 1, seed=11, wind=wind)
        _, ia, ib = np.intersect1d(ra['pid'], rb['pid'], return_indices=True)
        ok = (la[ia] == lb[ib]) & (ra['wp1'][ia, 2] < -0.05) & (rb['wp1'][ib, 2] < -0.05)
        ia, ib = ia[ok], ib[ok]
        if len(ia) == 0:
            continue
        vel, box = particles.field_kinematics(cam, dgrid, cdf, ra['pid'][ia], la[ia], 11, wind=wind)
        plain, _ = particles.field_kinematics(cam, dgrid, cdf, ra['pid'][ia], la[ia], 11)
        assert np.array_equal(vel[:, 0], plain[:, 0] + wind[0]) and np.array_equal(vel[:, 2], plain[:, 2] + wind[1])
        assert np.array_equal(vel[:, 1], plain[:, 1])
        r = (rb['wp1'][ib] - ra['wp1'][ia]) - vel * dt
        r[:, 0] -= box[:, 0] * np.rint(r[:, 0] / box[:, 0])
        r[:, 2] -= box[:, 2] * np.rint(r[:, 2] / box[:, 2])
        bound = cases._windy_bounds(cases._track_bounds(vel, box, la[ia], dt), vel, box, la[ia], dt)
        print('frame %d -> %d: %d kept again, worst |residual| / bound per axis %s' % (k, k + 1, len(ia), (np.abs(r) / bound).max(axis=0)))
        assert np.all(np.abs(r) <= bound), (np.abs(r) / bound).max(axis=0)
        total += len(ia)
    assert total >= 30, total


@pytest.mark.parametrize("wind", [(6.0, -2.0), (-7.5, 2.0)])
def test_rig_slots_move_by_the_windy_velocity(wind):
    """The rig-frame state (rig_state: what make_rig_slot makes) of every slot a stereo view keeps at k and k + 1 in one life."""
    rig = cases.KITTI_STEREO
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([50.0])})
    cam = particles.FrameCamera(opt, 0)
    box = rig.box(cam)
    _, dgrid, cdf, _ = particles.rig_expected_count(cam, 25, box)
    n_slots = int(particles.rig_slot_counts(opt, 25, 1, rig, seed=11)[0])
    dt = 1.0 / cam.hz
    total = 0
    for k in list(range(0, 6)) + list(range(1000, 1006)):
        sa = particles.rig_state(cam, dgrid, cdf, n_slots, k, 11, cam.hz, box, wind=wind)
        sb = particles.rig_state(cam, dgrid, cdf, n_slots, k + 1, 11, cam.hz, box, wind=wind)
        s0 = particles.rig_state(cam, dgrid, cdf, n_slots, k, 11, cam.hz, box)
        assert np.array_equal(sa['vel'][:, 0], s0['vel'][:, 0] + wind[0]) and np.array_equal(sa['vel'][:, 2], s0['vel'][:, 2] + wind[1])
        for v in range(len(rig)):
            ra, la = particles.rig_frame(opt, 25, k, rig, v, seed=11, wind=wind)
            rb, lb = particles.rig_frame(opt, 25, k + 1, rig, v, seed=11, wind=wind)
            _, ia, ib = np.intersect1d(ra['pid'], rb['pid'], return_indices=True)
            j = ra['pid'][ia[la[ia] == lb[ib]]]
            if len(j) == 0:
                continue
            assert np.array_equal(sa['life'][j], sb['life'][j])
            vel, w, wy = sa['vel'][j], 2.0 * sa['b'][j], 2.0 * sa['by'][j]
            r = (sb['pos'][j] - sa['pos'][j]) - vel * dt
            r[:, 0] -= w * np.rint(r[:, 0] / w)
            r[:, 2] -= w * np.rint(r[:, 2] / w)
            bound = cases._windy_bounds(cases._state_bounds(vel, w, wy, sa['life'][j], dt), vel, np.stack([w, wy, w], axis=1), sa['life'][j], dt)
            assert np.all(np.abs(r) <= bound), (np.abs(r) / bound).max(axis=0)
            total += len(j)
    print('%d tracks compared' % total)
    assert total >= 50, total


@pytest.mark.parametrize("name,model,rig", [('iid', 'iid', None), ('field', 'field', None), ('rig-ring', 'rig', cases.RING3)])
@pytest.mark.parametrize("wind", WINDS)
def test_a_streak_is_the_windy_velocity_times_the_exposure(sdb, name, model, rig, wind):
    """Every kept record: wpe - wps = R (vx, -v(D), vz) exposure in the view's axes (R = 1 for the i.i.d. and field models; the record
    stores depth = -z).  Bound, u = 2^-53: i.i.d. and field -- the end is fl(start + fl(velocity e)) with the product formed here
    with the same bits, then the test's subtraction: u |end| + u |end - start| per axis.  Rig -- the offset e_j = d_j + vel_j e carries
    2 u (|d_j| + |vel_j e|); each of the two rotations (three products, two sums) 3 u sum_j |R_ij| |.|_j <= 3 u |.|_2 (rows of unit
    length: Cauchy-Schwarz); the test's own R (vel e) another 3 u |vel e|_2 and its subtraction u: in all at most
    10 u (|wps|_2 + |vel e|_2) per axis.  (Records nearer than 5 cm are left out: their depth is clamped.)"""
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, None, [5])
    hz = float(opt['cam_hz'])
    tab = np.ascontiguousarray(cdf[0])
    recs = particles.expected_records(sims, dgrid, cdf, sdb, wind=wind, **kw)
    V = len(rig) if rig is not None else 1
    for i, s in enumerate(sims):
        table, _, W, H = particles._loaded_table(s, dgrid, cdf, sdb, 'kitti', model, hz, rig, i % V, wind=wind)
        pid = table.pid[h.hb.filter_streaks(table, W, H)]
        rec = recs[i]
        assert len(pid) == len(rec) > 100
        allp, life = _all_particles(model, cam, dgrid, tab, s, hz, rig, None, i % V, box, wind)
        D = allp['wd1'][pid] * 1e3
        v = particles.terminal_velocity(D)
        seed = int(s['key0']) | (int(s['key1']) << 32)
        if model == 'iid':
            own = particles._block_wind(particles.philox4x32(pid.astype(np.uint64), int(s['frame']), 2, 0, *particles._key(seed)), 1.0)
        else:
            own = particles._block_wind(particles.philox4x32(*particles._life_counter(pid.astype(np.uint64), life[pid], 2), *particles._key(seed)), 1.0)
        vel = np.stack([own + wind[0], -v, np.full(len(pid), cam.speed + wind[1])], axis=1)
        R = np.eye(3) if rig is None else np.asarray(rig.views[i % V][0], np.float64).reshape(3, 3)
        want = (vel * cam.exposure) @ R.T
        want[:, 2] = -want[:, 2]                                   # the record's z is the depth
        got = rec['wpe'] - rec['wps']
        free = rec['wps'][:, 2] > 0.05
        if rig is None:
            bound = U * (np.abs(rec['wpe']) + np.abs(got)) + 2.0 * U * np.abs(want)      # (v(D) from wd 1e3: D itself to a relative 2 u)
        else:
            bound = (10.0 * U * (np.sqrt((rec['wps'] ** 2).sum(axis=1)) + np.sqrt((want ** 2).sum(axis=1))))[:, None] * np.ones(3)
        bound[:, 1] += 4.0 * U * np.abs(want[:, 1])                # v(D) of the D read back from the record's diameter in metres
        err = np.abs(got - want)[free]
        print('%s view %d: worst |error| / bound per axis %s' % (name, i % V, (err / bound[free]).max(axis=0)))
        assert np.all(err <= bound[free]), (err / bound[free]).max(axis=0)
        assert free.sum() > 100


# ---- 4. the law ----------------------------------------------------------------------------------------------------
def test_a_windy_field_frame_has_the_iid_models_law():
    wind = (6.0, -2.0)
    opt = cases.options('kitti')
    cam = particles.FrameCamera(opt, 0)
    counts, D, depth, px, py = [], [], [], [], []
    for i in range(cases.N_LAW):                                  # cases._sample('field', 9000) with the wind
        rec, _ = particles.field_frame(opt, 25, 7 * i + 3, seed=9000 + i, wind=wind)
        counts.append(len(rec))
        D.append(rec['wd1'] * 1e3)
        depth.append(-rec['wp1'][:, 2])
        px.append(rec['ip1'][:, 0])
        py.append(rec['ip1'][:, 1])
    field = dict(cam=cam, counts=np.array(counts), D=np.concatenate(D), depth=np.concatenate(depth), px=np.concatenate(px), py=np.concatenate(py))
    iid_a, iid_b = cases._sample('iid', 1000), cases._sample('iid', 5000)
    control = cases._same_law(iid_a, iid_b)
    assert all(v < 1 for v in control.values()), control
    mean = particles.expected_count(cam, 25)[0]
    assert abs(field['counts'].mean() - mean) < 4 * np.sqrt(mean / cases.N_LAW)
    got, got_b = cases._same_law(field, iid_a), cases._same_law(field, iid_b)
    print('statistic / threshold -- iid vs iid: %s\n  windy field vs iid: %s\n  windy field vs iid (other seeds): %s' % (control, got, got_b))
    assert all(v < 1 for v in got.values()), got
    assert all(v < 1 for v in got_b.values()), got_b
    # and the frames are not the calm ones
    calm, _ = particles.field_frame(opt, 25, 3, seed=9000)
    windy, _ = particles.field_frame(opt, 25, 3, seed=9000, wind=wind)
    assert calm['pid'].tobytes() != windy['pid'].tobytes()


# ---- 5. slant ------------------------------------------------------------------------------------------------------
def _calm_records(sdb, model, rig, traj, wind, frames=(4,)):
    """Records with no scatter (wind_sigma 0) and no ego-motion, and per record the terminal velocity of its drop."""
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, list(frames), speed_kmh=0.0)
    sims['wind_sigma'] = 0.0
    hz = float(opt['cam_hz'])
    recs = particles.expected_records(sims, dgrid, cdf, sdb, wind=wind, **kw)
    V = len(rig) if rig is not None else 1
    vs = []
    for i, s in enumerate(sims):
        table, _, W, H = particles._loaded_table(s, dgrid, cdf, sdb, 'kitti', model, hz, rig, i % V, trajectory=traj, wind=wind)
        pid = table.pid[h.hb.filter_streaks(table, W, H)]
        D = particles._slot_draw(cam, dgrid, cdf[0], pid.astype(np.uint64), particles._key(SEED), 1.0, 15.0)[0] if model != 'iid' else \
            particles.sample_diameter(dgrid, cdf[0], particles.unit32(particles.philox4x32(pid.astype(np.uint64), int(s['frame']), 0, 0,
                                                                                             *particles._key(SEED))[0]))
        assert len(pid) == len(recs[i]) > 100
        vs.append(particles.terminal_velocity(D))
    return recs, vs, cam, sims


@pytest.mark.parametrize("model", ['iid', 'field'])
@pytest.mark.parametrize("wx", [5.0, -7.5])
def test_streaks_lean_the_winds_way_by_wx_over_v(sdb, model, wx):
    """No scatter, no ego-motion, wz = 0: the depth does not change over the exposure, so the projected streak is (wx, v) e fpx / depth
    exactly and dx / dy = wx / v(D).  Each end point is rounded to a pixel (half a pixel each): |dx - (wx / v) dy| <= 1 + |wx / v|."""
    recs, vs, _, _ = _calm_records(sdb, model, None, None, (wx, 0.0))
    for rec, v in zip(recs, vs):
        dx, dy = (rec['x1'] - rec['x0']).astype(np.float64), (rec['y1'] - rec['y0']).astype(np.float64)
        assert np.all(dx >= 0) if wx > 0 else np.all(dx <= 0)
        assert np.all(dy >= 0)                                    # they fall: the image's y grows downward
        nb = rec['type'] != 0
        r = wx / v
        err = np.abs(dx - r * dy)
        print('%s wx %+.1f: %d non-Big records, slopes %.2f .. %.2f, worst |dx - r dy| / (1 + |r|) %.3f'
              % (model, wx, nb.sum(), np.abs(r[nb]).min(), np.abs(r[nb]).max(), (err / (1.0 + np.abs(r)))[nb].max()))
        assert nb.sum() > 100 and np.all(err[nb] <= (1.0 + np.abs(r[nb])) * (1.0 + 1e-12))
        assert np.abs(dx[nb]).max() >= 3                          # visibly slanted
        # small drops lean more than large ones: wx / v(D) falls with D
        assert np.all(np.diff(np.abs(r)[np.argsort(v)]) <= 0)


def test_a_view_yawed_180_degrees_sees_the_opposite_lean(sdb):
    recs, _, _, _ = _calm_records(sdb, 'rig', cases.BACK_TO_BACK, None, (5.0, 0.0))
    front, back = recs[0], recs[1]
    assert np.all(front['x1'] >= front['x0']) and np.all(back['x1'] <= back['x0'])
    assert (front['x1'] > front['x0']).sum() > 100 and (back['x1'] < back['x0']).sum() > 100


def test_under_a_trajectory_the_wind_is_a_world_vector(sdb):
    """A rig that stands yawed by 90 degrees (it looks along the world's -x): the world's wind (wx, 0) blows along the rig's own +z,
    toward the viewer -- the streak's x extent in the camera is rounding only, its depth shrinks by wx e."""
    wx = 5.0
    traj = trajmod.Trajectory(np.array([cases.pose(90.0), cases.pose(90.0)]), 10.0, 'native')
    recs, vs, cam, _ = _calm_records(sdb, 'rig', cases.MONO, traj, (wx, 0.0), frames=(0,))
    rec = recs[0]
    free = rec['wps'][:, 2] > 0.05
    d = (rec['wpe'] - rec['wps'])[free]
    scale = np.sqrt((rec['wps'][free] ** 2).sum(axis=1)) + wx * cam.exposure
    assert np.all(np.abs(d[:, 0]) <= 1e-15 * scale + 7e-17 * wx * cam.exposure)        # cos(90 deg) in double is 6.1e-17, not 0
    assert np.all(np.abs(d[:, 2] + wx * cam.exposure) <= 10.0 * U * scale)
    assert np.all(np.abs(d[:, 1] + vs[0][free] * cam.exposure) <= 10.0 * U * scale + 4.0 * U * vs[0][free] * cam.exposure)
    # the same wind on the rig at rest (no trajectory) blows along the rig's x
    rest, _, _, _ = _calm_records(sdb, 'rig', cases.MONO, None, (wx, 0.0))
    d0 = rest[0]['wpe'] - rest[0]['wps']
    assert np.all(np.abs(d0[:, 0] - wx * cam.exposure) <= 10.0 * U * (np.abs(rest[0]['wps']).sum(axis=1) + 1.0)) and np.all(d0[:, 2] == 0)


# ---- 8. refusals, the public interface -----------------------------------------------------------------------------
def test_refusals(tmp_path, sdb):
    opt = cases.options('kitti')
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1)
    for bad in ((float('nan'), 0.0), (0.0, float('inf')), (100.5, 0.0), (0.0, -101.0), (1.0,), (1.0, 2.0, 3.0), 'wind', None, ('a', 'b')):
        with pytest.raises(ValueError, match='wind'):
            particles.expected_records(sims, dgrid, cdf, sdb, wind=bad)
    particles.expected_records(sims[:0], dgrid, cdf, sdb, wind=(100.0, -100.0))     # the limit itself is allowed
    with pytest.raises(ValueError, match='wind'):
        particles.make_particles(particles.FrameCamera(opt, 0), dgrid, cdf[0], 4, 0, 0, wind=(float('nan'), 0.0))
    # angular noise stays where it is allowed today: the i.i.d. model, with a wind too
    run = ([0], [0])
    noisy = sims.copy()
    noisy['run_pos'] = 1
    a = particles.expected_records(noisy, dgrid, cdf, sdb, noise_std=2.0, noise_scale=1.0, run=run, wind=(3.0, 0.0))
    b = particles.expected_records(noisy, dgrid, cdf, sdb, noise_std=2.0, noise_scale=1.0, run=run)
    assert len(a[0]) > 100 and a[0].tobytes() != b[0].tobytes()
    with pytest.raises(ValueError, match='no angular noise'):
        particles.expected_records(sims, dgrid, cdf, sdb, model='field', cam_hz=10.0, noise_std=2.0, noise_scale=1.0, wind=(3.0, 0.0))
    # the driver's argument handling (before it looks at any path)
    main = importlib.import_module('rain-rendering_amd.main')
    common = ['--dataset', 'kitti', '-k', str(tmp_path), '-i', '25']
    with pytest.raises(SystemExit, match='--wind needs --device_particles'):
        main._derive(main._parse(common + ['--wind', '5,0']))
    for bad in ('5', '5,0,1', 'a,b', 'nan,0', '0,101', ''):
        with pytest.raises(SystemExit, match='--wind'):
            main._derive(main._parse(common + ['--wind=' + bad, '--device_particles']))
    with pytest.raises(SystemExit):
        main._parse(common + ['--streak_lean', 'maybe'])
    ns = main._parse(common)
    assert ns.wind is None and ns.streak_lean == 'auto'
    assert main._parse(common + ['--wind=-7.5,2', '--streak_lean', 'off']).streak_lean == 'off'


def test_streak_lean_auto_follows_the_wind(tmp_path):
    """--streak_lean auto is on exactly when a non-zero wind is given: no command line without --wind changes its output."""
    main = importlib.import_module('rain-rendering_amd.main')
    common = ['--dataset', 'kitti', '-k', str(tmp_path), '-i', '25']

    def lean(extra):
        ns = main._wind_and_lean(main._parse(common + extra))
        return ns.wind, ns.lean
    assert lean([]) == ((0.0, 0.0), False)
    assert lean(['--device_particles']) == ((0.0, 0.0), False)
    assert lean(['--device_particles', '--wind=0,0']) == ((0.0, 0.0), False)
    assert lean(['--device_particles', '--wind=5,0']) == ((5.0, 0.0), True)
    assert lean(['--device_particles', '--wind=0,-2.5']) == ((0.0, -2.5), True)
    assert lean(['--device_particles', '--wind=5,0', '--streak_lean', 'off']) == ((5.0, 0.0), False)
    assert lean(['--streak_lean', 'on']) == ((0.0, 0.0), True)


def test_rain_augment_plan_carries_the_wind(tmp_path):
    augment = importlib.import_module('rain-rendering_amd.augment')
    root = str(tmp_path)
    h.synthetic.write_streak_db(os.path.join(root, 'rainstreakdb'))
    kw = dict(streaks_db=os.path.join(root, 'rainstreakdb'), sequence='data_object/training')
    aug = augment.RainAugment('kitti', particle_model='field', draws='counter', wind=(6, 0), **kw)
    p = aug.plan(25, [4, 11])
    assert p['wind'] == (6.0, 0.0) and p['lean'] is True
    calm = augment.RainAugment('kitti', particle_model='field', draws='counter', **kw)
    assert calm.plan(25, [4])['wind'] == (0.0, 0.0) and calm.plan(25, [4])['lean'] is False
    assert augment.RainAugment('kitti', wind=(6, 0), lean=False, **kw).lean is False
    assert augment.RainAugment('kitti', lean=True, **kw).lean is True
    recs = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, model='field', cam_hz=p['cam_hz'], draws=p['draws'],
                                      wind=p['wind'])
    plain = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, model='field', cam_hz=p['cam_hz'], draws=p['draws'])
    assert len(recs[0]) > 100 and recs[0].tobytes() != plain[0].tobytes()
    for bad in ((float('nan'), 0), (0, 200.0), 5.0, (1, 2, 3), 'ab', (True, 0), None):
        with pytest.raises(ValueError, match='wind'):
            augment.RainAugment('kitti', wind=bad, **kw)
    for bad in (1, 'on', 0.0):
        with pytest.raises(ValueError, match='lean'):
            augment.RainAugment('kitti', lean=bad, **kw)
