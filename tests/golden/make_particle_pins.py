"""Pins the bits of the rain-particle model's numpy statement (rain-rendering_amd/tools/particles.py).

    python tests/golden/make_particle_pins.py        # writes tests/golden/particle_pins.json

The host tests assert that the numpy statement and the g++ build of rr_particles.h are EQUAL; a change made the same way on
both sides passes them.  `digests()` computes SHA-256 digests of the raw bytes of what the statement returns -- every model
(i.i.d., field, rig, rig under a trajectory), both draw modes, with and without jitter, angular noise -- at the small shapes of
tests/test_particle_*_host.py, and tests/test_particle_pins.py compares them with the committed file.

The committed particle_pins.json was written by this script on the tree of commit 019af6a ("Add camera trajectories: the
rig's rain field from a moving, turning rig"), BEFORE the slot / view / store steps of the model were folded into shared
helpers.  Regenerate it only where a change of the model's bits is the purpose of a change.

NaN rotation terms (a streak of zero length: 0 / 0) are stored as one canonical NaN before hashing: their sign and payload are
the machine's (tests/test_particle_jitter_host.py _same_field).
"""
import hashlib
import importlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, 'particle_pins.json')
TIMES = (0, 3, 2 ** 31 + 5)                    # time indices: 0, a small one, one at which the slots' lives differ widely
SEED = 1234 + 2 ** 40                          # (both key words non-zero)
JITTER = 5.0


def _canon(a):
    """`a` with every NaN of its float fields replaced by numpy's own."""
    a = np.array(a)                             # a contiguous copy
    if a.dtype.names:
        for nm in a.dtype.names:
            if a.dtype[nm].base.kind == 'f':
                f = a[nm]
                f[np.isnan(f)] = np.nan
    elif a.dtype.kind == 'f':
        a[np.isnan(a)] = np.nan
    return a


def _sha(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(_canon(a))
        m.update(('%s%s;' % (a.dtype.str if not a.dtype.names else 'rec', a.shape)).encode())
        m.update(a.tobytes())
    return m.hexdigest()


def _pose(rigmod, yaw_deg, pitch_deg, t):
    P = np.zeros((3, 4))
    P[:, :3] = rigmod._rot_y(yaw_deg) @ rigmod._rot_x(pitch_deg)
    P[:, 3] = t
    return P


def _trajectory(rigmod, trajmod):
    """Instants 0, 2, 4, 6: yaw 0, 90, 180, 37 degrees (the last two pitched), 0 .. 1e5 m from the origin; each is followed by a
    pose 2 degrees and a few decimetres further: the camera moves and turns during the exposure."""
    poses = []
    for yaw, pitch, dist in [(0.0, 0.0, 0.0), (90.0, 0.0, 1e3), (180.0, 7.0, 1e5), (37.0, -4.0, 1e5)]:
        d = np.array([0.6, 0.0, -0.8]) * dist
        poses.append(_pose(rigmod, yaw, pitch, d))
        poses.append(_pose(rigmod, yaw + 2.0, pitch + 0.5, d + np.array([0.3, 0.02, -0.9])))
    return trajmod.Trajectory(np.array(poses), 10.0, 'native')


def _run(particles, model, opt, rate, frames, seed, rig=None, count=None, trajectory=None):
    """tests/test_particle_draws_host.py _run: (sims of the rendered frames, d_grid, cdf, expected_records' keywords)."""
    sims, dgrid, cdf = particles.sim_frames(opt, rate, 1, seed=seed, model=model, rig=rig, count=count, trajectory=trajectory)
    kw = dict(model=model)
    if model == 'iid':
        sims = np.ascontiguousarray(sims[np.zeros(len(frames), np.int64)])
        sims['frame'] = np.asarray(frames, np.uint32)
        sims['draw_seed'] = np.asarray(frames, np.uint32)
    elif model == 'field':
        sims = particles.field_run_sims(sims, frames)
        kw.update(cam_hz=opt['cam_hz'])
    else:
        sims = particles.rig_run_sims(sims, frames, len(rig))
        kw.update(cam_hz=opt['cam_hz'], rig=rig)
        if trajectory is not None:
            kw.update(trajectory=trajectory)
    return sims, dgrid, cdf, kw


def digests():
    """{name: SHA-256 hex digest} of the numpy statement's arrays."""
    import helpers as h
    particles = importlib.import_module('rain-rendering_amd.tools.particles')
    rigmod = importlib.import_module('rain-rendering_amd.rig')
    trajmod = importlib.import_module('rain-rendering_amd.trajectory')
    db = importlib.import_module('rain-rendering_amd.common.db')

    def options(**kw):
        o = dict(db.settings('kitti'))
        o.pop('sequences', None)
        o.update(kw)
        return o

    out = {}
    opt = options(sim_steps={"cam_motion": np.array([30.0])})
    cam = particles.FrameCamera(opt, 0)
    hz = float(opt['cam_hz'])
    stereo = rigmod.Rig.stereo(0.54)
    ring6 = rigmod.Rig.yaw_ring([0, 55, 110, 180, -110, -55], 0.8)
    traj = _trajectory(rigmod, trajmod)

    # ---- the generators -------------------------------------------------------------------------------------------
    _, dgrid, cdf, z_max = particles.expected_count(cam, 25)
    out['expected_count'] = _sha(dgrid, cdf, z_max)
    for k in TIMES:
        out['make_particles/k%d' % k] = _sha(particles.make_particles(cam, dgrid, cdf, 1500, k, SEED))
        full, life = particles.make_field_particles(cam, dgrid, cdf, 2000, k, SEED, hz, cull=False)
        kept, klife = particles.make_field_particles(cam, dgrid, cdf, 2000, k, SEED, hz, cull=True)
        assert 100 < len(kept) < len(full)
        out['make_field_particles/k%d/all' % k] = _sha(full, life)
        out['make_field_particles/k%d/culled' % k] = _sha(kept, klife)
        vel, boxes = particles.field_kinematics(cam, dgrid, cdf, np.arange(2000), life, SEED)
        out['field_kinematics/k%d' % k] = _sha(vel, boxes)
        pid = np.arange(2000)
        out['counter_picks/frame/k%d' % k] = _sha(particles.counter_picks(SEED, pid, frame=k))
        out['counter_picks/life/k%d' % k] = _sha(particles.counter_picks(SEED, pid, life=life))
        out['counter_jitter/frame/k%d' % k] = _sha(particles.counter_jitter(SEED, pid, frame=k))
        out['counter_jitter/life/k%d' % k] = _sha(particles.counter_jitter(SEED, pid, life=life))
    assert len(set(life.tolist())) > 100                      # the lives differ between slots at the last time index
    for name, rig in (('stereo', stereo), ('ring6', ring6)):
        box = tuple(float(v) for v in rig.box(cam))
        _, rgrid, rcdf, rz = particles.rig_expected_count(cam, 25, box)
        out['rig_expected_count/%s' % name] = _sha(rgrid, rcdf, rz)
        tcam = particles._traj_cam(cam)
        tbox = tuple(float(v) for v in traj.box(rig, tcam))
        poses = traj.compose(rig, tcam.exposure)
        for n_k, k in enumerate(TIMES):
            st = particles.rig_state(cam, rgrid, rcdf, 1800, k, SEED, hz, box)
            out['rig_state/%s/k%d' % (name, k)] = _sha(*[np.asarray(st[key]) for key in sorted(st)])
            for v in range(len(rig)):
                for cull in (False, True):
                    rec, lf = particles.make_rig_particles(cam, rgrid, rcdf, 1800, k, SEED, hz, rig.views[v], box, cull=cull)
                    out['make_rig_particles/%s/k%d/v%d/%s' % (name, k, v, 'culled' if cull else 'all')] = _sha(rec, lf)
                    po = poses[2 * (n_k + 1), v]               # instants 2, 4, 6: a moving, turning view far from the origin
                    assert po['R0'].tobytes() != po['R1'].tobytes() and po['c0'].tobytes() != po['c1'].tobytes()
                    rec, lf = particles.make_rig_particles(tcam, rgrid, rcdf, 1800, k, SEED, hz, (po['R0'], po['c0']), tbox, cull=cull,
                                                           view_end=(po['R1'], po['c1']))
                    out['make_rig_particles/%s/k%d/v%d/%s/view_end' % (name, k, v, 'culled' if cull else 'all')] = _sha(rec, lf)

    # ---- a run whose simulated frames change the fall rate (and the speed) --------------------------------------------------
    ropt = options(sim_mode='steps', sim_steps={"rain_fallrate": np.array([10.0, 25.0, 25.0, 50.0, 10.0]),
                                                "cam_motion": np.array([30.0, 30.0, 50.0, 50.0, 30.0])})
    for count in (None, 700):
        tag = 'poisson' if count is None else 'count'
        out['frame_counts/' + tag] = _sha(particles.frame_counts(ropt, 25, 5, seed=SEED, count=count))
        out['field_slot_counts/' + tag] = _sha(particles.field_slot_counts(ropt, 25, 5, seed=SEED, count=count))
        for name, rig in (('stereo', stereo), ('ring6', ring6)):
            out['rig_slot_counts/%s/%s' % (name, tag)] = _sha(particles.rig_slot_counts(ropt, 25, 5, rig, seed=SEED, count=count))
    out['diameter_tables'] = _sha(*particles.diameter_tables(ropt, 25, 5))
    for name, rig in (('stereo', stereo), ('ring6', ring6)):
        out['rig_tables/' + name] = _sha(*particles.rig_tables(ropt, 25, 5, rig))
    for model, rig in (('iid', None), ('field', None), ('rig', stereo)):
        sims, g, c = particles.sim_frames(ropt, 25, 5, seed=SEED, model=model, rig=rig)
        out['sim_frames/' + model] = _sha(sims, g, c)

    # ---- the finished records -------------------------------------------------------------------------------------------
    with tempfile.TemporaryDirectory() as tmp:
        sdb = h.Scene(tmp, 64, 96, 10).db                       # the streak database of the host tests (texture ratios)
        runs = [('iid', 'iid', None, None, list(TIMES)), ('field', 'field', None, None, list(TIMES)),
                ('rig', 'rig', stereo, None, list(TIMES)), ('rig-traj', 'rig', stereo, traj, [0, 2, 6])]
        for name, model, rig, trajectory, frames in runs:
            sims, g, c, kw = _run(particles, model, opt, 25, frames, SEED, rig, count=600, trajectory=trajectory)
            for draws in ('stream', 'counter'):
                for jitter in (0.0, JITTER):
                    recs = particles.expected_records(sims, g, c, sdb, draws=draws, jitter=jitter, **kw)
                    assert all(len(r) > 50 for r in recs), (name, [len(r) for r in recs])
                    out['expected_records/%s/%s/jitter%g' % (name, draws, jitter)] = _sha(*recs)
        # the i.i.d. model with angular noise and a run (tests/test_particle_noise_host.py)
        nopt = options()
        sims, g, c = particles.sim_frames(nopt, 100, 2, seed=11, count=800)
        f_idx = list(range(5))
        run = particles.run_table(sims, len(sims), f_idx)
        fr = sims[np.asarray(f_idx) % len(sims)].copy()
        fr['draw_seed'] = f_idx
        fr['run_pos'] = np.arange(1, len(f_idx) + 1)
        recs = particles.expected_records(fr, g, c, sdb, noise_std=3.0, noise_scale=1.0, run=run)
        out['expected_records/iid/noise'] = _sha(*recs)
    return out


def main():
    d = digests()
    with open(OUT, 'w') as fh:
        json.dump(d, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print('%d digests -> %s' % (len(d), OUT))


if __name__ == '__main__':
    main()
