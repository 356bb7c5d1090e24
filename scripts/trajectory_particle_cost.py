"""Cost of a camera trajectory under the rig particle model (rr_set_particle_trajectory, k_rig_particles<.., TRAJ = true>) against the
same rig without one: the particle kernel's own time from the library profile (rr_profile_read) for rr_generate_drops_device.
Three legs in interleaved rounds inside one process: `rig` (the rig's own box, no trajectory: the parent's kernel and workload),
`rig_wide` (no trajectory, but the box and slot count of the trajectory: what the wider box alone costs) and `traj` (that box
with the trajectory: what reading the poses from the table costs on top).  The trajectory is an arc (10 m/s, 20 deg/s) with one
pose per instant of the batch.  Median / minimum / maximum over the rounds.  Prints one JSON line per batch size.

  python scripts/trajectory_particle_cost.py [--workload kitti25] [--rig stereo:0.54 | ring6 | mono] [--frames 8,32,128,512] [--rounds 7] [--calls 5]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='kitti25')
    ap.add_argument('--rig', default='stereo:0.54', help="'mono', 'stereo:<m>', 'ring6' (six yaws, 0.8 m) or a JSON file")
    ap.add_argument('--frames', default='8,32,128,512', help='frames per call (instants x views, rounded down to whole instants)')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    hb = importlib.import_module('rain-rendering_amd.hip_backend')
    particles = importlib.import_module('rain-rendering_amd.tools.particles')
    rigmod = importlib.import_module('rain-rendering_amd.rig')
    db = importlib.import_module('rain-rendering_amd.common.db')
    bw = importlib.import_module('rain-rendering_amd.common.bad_weather')
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    tmp = tempfile.mkdtemp()
    tex_dir, norm = synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
    streaks = bw.DBManager(streaks_path=tex_dir, norm_coeff_path=norm)
    streaks.load_streak_database()
    wl = a.workload
    dataset, rate = wl.rstrip('0123456789'), int(wl[len(wl.rstrip('0123456789')):])
    opts = {k: v for k, v in db.settings(dataset).items() if k != 'sequences'}
    rig = rigmod.Rig.yaw_ring([0, 55, 110, 180, -110, -55], 0.8) if a.rig == 'ring6' else rigmod.Rig.from_spec(a.rig)
    V = len(rig)
    W, H = (int(v) for v in opts['cam_CCD_WH'])
    trajmod = importlib.import_module('rain-rendering_amd.trajectory')
    n_max = max(max(int(b) for b in a.frames.split(',')) // V, 1)
    om, hz = np.deg2rad(20.0), float(opts['cam_hz'])
    rad = 10.0 / om
    poses = np.zeros((n_max + 1, 3, 4))
    for k in range(n_max + 1):
        psi = om * k / hz
        poses[k, :, :3] = rigmod._rot_y(np.rad2deg(psi))
        poses[k, :, 3] = (-rad + rad * np.cos(psi), 0.0, -rad * np.sin(psi))
    traj = trajmod.Trajectory(poses, hz)
    opts = dict(opts, sim_steps={})                              # no ego-motion in any leg: the same drops' motion, the same work
    cam = particles.FrameCamera(opts, 0)
    s_rig, dgrid, cdf_rig = particles.sim_frames(opts, rate, 1, seed=0, model='rig', rig=rig)
    s_wide, _, cdf_wide = particles.sim_frames(opts, rate, 1, seed=0, model='rig', rig=rig, trajectory=traj)
    s_wide['table'] = 1                                          # one context, both tables
    cdf = np.concatenate([np.atleast_2d(cdf_rig), np.atleast_2d(cdf_wide)])
    cap = int(particles.sim_frames(opts, rate, 1, seed=0)[0]['n_particles'].max()) * 2
    box_rig, box_wide = rig.box(cam), traj.box(rig, cam)
    table = traj.compose(rig, cam.exposure)
    rh = hb.RainHip(0)
    rh.set_streak_db(streaks.streaks_light)
    rh.set_particle_tables(dgrid, cdf)
    for F in (int(b) for b in a.frames.split(',')):
        n_inst = max(F // V, 1)
        B = n_inst * V
        drops = torch.empty((B, cap * hb.DROP_DTYPE.itemsize), dtype=torch.uint8, device='cuda:0')
        counts = torch.empty(B, dtype=torch.int32, device='cuda:0')
        inst = np.arange(n_inst)
        frames = {'rig': particles.rig_run_sims(s_rig, inst, V), 'rig_wide': particles.rig_run_sims(s_wide, inst, V)}
        frames['traj'] = frames['rig_wide']
        per = {'rig': [], 'rig_wide': [], 'traj': []}
        kept = {}

        def one(leg, timed):
            rh.set_particle_rig(rig.as_records(), box_rig if leg == 'rig' else box_wide)
            rh.set_particle_model('rig', opts['cam_hz'])
            rh.set_particle_trajectory(table if leg == 'traj' else None)
            rh.profile(True)
            rh.profile_reset()
            for _ in range(a.calls):
                rh.generate_drops_device(frames[leg], H, W, drops.data_ptr(), cap, counts.data_ptr())
            torch.cuda.synchronize()
            st = rh.profile_read()
            rh.profile(False)
            kept[leg] = float(counts.cpu().numpy().mean())
            if timed:
                per[leg].append(st['k_rig_particles'][1] / a.calls)
        for leg in per:
            one(leg, False)
        for _ in range(a.rounds):
            for leg in per:
                one(leg, True)
        res = dict(workload=wl, rig=a.rig, views=V, instants=n_inst, frames_per_call=B, rounds=a.rounds, calls_per_round=a.calls,
                   unit='ms per call (all views)', kept_per_frame={m: round(v, 1) for m, v in kept.items()},
                   slots={'rig': int(s_rig['n_particles'].max()), 'trajectory_box': int(s_wide['n_particles'].max())},
                   box={'rig': [round(v, 4) for v in box_rig], 'trajectory': [round(v, 4) for v in box_wide]},
                   k_rig=_stats(per['rig']), k_rig_wide=_stats(per['rig_wide']), k_traj=_stats(per['traj']))
        res['traj_over_rig_wide'] = round(res['k_traj']['median'] / res['k_rig_wide']['median'], 3)
        res['traj_over_rig'] = round(res['k_traj']['median'] / res['k_rig']['median'], 3)
        print(json.dumps(res), flush=True)
        del drops, counts
    rh.close()


if __name__ == '__main__':
    main()
