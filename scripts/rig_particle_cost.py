"""Cost of the rig particle model (rr_set_particle_rig, k_rig_particles) against the field model launched once per view: the
particle kernels' own time from the library profile (rr_profile_read) for rr_generate_drops_device on one workload.  The fused
kernel evaluates a slot's rig-frame state once and walks the views; the baseline is what a user had before it: V calls under
the field model (k_field_particles, unchanged by the rig model) with the same instants, one per camera.  Both in interleaved
rounds inside one process; median / minimum / maximum over the rounds.  Prints one JSON line per batch size.

  python scripts/rig_particle_cost.py [--workload kitti25] [--rig stereo:0.54 | ring6] [--frames 8,32,128,512] [--rounds 7] [--calls 5]
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
    ap.add_argument('--rig', default='stereo:0.54', help="'stereo:<m>', 'ring6' (six yaws, 0.8 m) or a JSON file")
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
    s_field, dgrid, cdf_field = particles.sim_frames(opts, rate, 1, seed=0, model='field')
    s_rig, _, cdf_rig = particles.sim_frames(opts, rate, 1, seed=0, model='rig', rig=rig)
    s_rig['table'] = 1                                           # one context, both tables
    cdf = np.concatenate([np.atleast_2d(cdf_field), np.atleast_2d(cdf_rig)])
    cap = int(s_field['n_particles'].max())
    rh = hb.RainHip(0)
    rh.set_streak_db(streaks.streaks_light)
    rh.set_particle_tables(dgrid, cdf)
    rh.set_particle_rig(rig.as_records(), rig.box(particles.FrameCamera(opts, 0)))
    for F in (int(b) for b in a.frames.split(',')):
        n_inst = max(F // V, 1)
        B = n_inst * V
        drops = torch.empty((B, cap * hb.DROP_DTYPE.itemsize), dtype=torch.uint8, device='cuda:0')
        counts = torch.empty(B, dtype=torch.int32, device='cuda:0')
        inst = np.arange(n_inst)
        frames = {'rig': particles.rig_run_sims(s_rig, inst, V), 'field': particles.field_run_sims(s_field, inst)}
        per = {'rig': [], 'field': []}
        kept = {}

        def one(leg, timed):
            rh.set_particle_model(leg, opts['cam_hz'])
            rh.profile(True)
            rh.profile_reset()
            for _ in range(a.calls):
                if leg == 'rig':
                    rh.generate_drops_device(frames['rig'], H, W, drops.data_ptr(), cap, counts.data_ptr())
                else:                                            # one call per camera, each into its own part of the buffer
                    for v in range(V):
                        rh.generate_drops_device(frames['field'], H, W, drops.data_ptr() + v * n_inst * cap * hb.DROP_DTYPE.itemsize, cap,
                                                 counts.data_ptr() + 4 * v * n_inst)
            torch.cuda.synchronize()
            st = rh.profile_read()
            rh.profile(False)
            kept[leg] = float(counts.cpu().numpy().mean())
            if timed:
                per[leg].append(st['k_rig_particles' if leg == 'rig' else 'k_field_particles'][1] / a.calls)
        for leg in per:
            one(leg, False)
        for _ in range(a.rounds):
            for leg in per:
                one(leg, True)
        res = dict(workload=wl, rig=a.rig, views=V, instants=n_inst, frames_per_call=B, rounds=a.rounds, calls_per_round=a.calls,
                   unit='ms per call (all views)', kept_per_frame={m: round(v, 1) for m, v in kept.items()},
                   slots={'rig': int(s_rig['n_particles'].max()), 'field_per_view': int(s_field['n_particles'].max())},
                   k_rig_particles=_stats(per['rig']), k_field_particles_x_views=_stats(per['field']))
        res['rig_over_field'] = round(res['k_rig_particles']['median'] / res['k_field_particles_x_views']['median'], 3)
        print(json.dumps(res), flush=True)
        del drops, counts
    rh.close()


if __name__ == '__main__':
    main()
