"""Cost of angular noise (--noise_std) on device-generated drop tables: rr_generate_drops_device over a run of 4 * n_sim
frames (frame f: simulated frame f % n_sim, seed f, run entry f -- the driver's run), in calls of --batch frames, noise off
against noise on.  Prints one JSON line per workload.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/noise_generation_cost.py`.

  python scripts/noise_generation_cost.py [--workloads kitti100,nuscenes100] [--batch 512] [--repeat 3]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='kitti100,nuscenes100')
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--noise_std', type=float, default=3.0)
    ap.add_argument('--noise_scale', type=float, default=1.0)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    hb = importlib.import_module('rain-rendering_amd.hip_backend')
    particles = importlib.import_module('rain-rendering_amd.tools.particles')
    db = importlib.import_module('rain-rendering_amd.common.db')
    bw = importlib.import_module('rain-rendering_amd.common.bad_weather')
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    tmp = tempfile.mkdtemp()
    tex_dir, norm = synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
    streaks = bw.DBManager(streaks_path=tex_dir, norm_coeff_path=norm)
    streaks.load_streak_database()
    for wl in a.workloads.split(','):
        dataset, rate = wl.rstrip('0123456789'), int(wl[len(wl.rstrip('0123456789')):])
        # KITTI's one sequence (data_object) is simulated in 101 steps; nuScenes with the dataset's settings
        opts = db.sim(dataset, 'data_object', tmp)['options'] if dataset == 'kitti' else \
            {k: v for k, v in db.settings(dataset).items() if k != 'sequences'}
        n_sim = particles.n_sim_frames(opts)
        sims, dgrid, cdf = particles.sim_frames(opts, rate, n_sim, seed=0)
        W, H = (int(v) for v in opts['cam_CCD_WH'])
        n = 4 * n_sim
        f_idx = np.arange(n)
        run_frame, run_seed = particles.run_table(sims, n_sim, f_idx)
        frames = sims[f_idx % n_sim].copy()
        frames['draw_seed'] = f_idx
        cap = int(sims['n_particles'].max())
        B = min(a.batch, n)
        rh = hb.RainHip(0)
        rh.set_streak_db(streaks.streaks_light)
        rh.set_particle_tables(dgrid, cdf)
        drops = torch.empty((B, cap * hb.DROP_DTYPE.itemsize), dtype=torch.uint8, device='cuda:0')
        counts = torch.empty(B, dtype=torch.int32, device='cuda:0')
        res = dict(workload=wl, n_sim=n_sim, frames=n, frames_per_call=B, drops_per_frame_mean=None)
        for noisy in (False, True):
            fr = frames.copy()
            fr['run_pos'] = f_idx + 1 if noisy else 0
            times, kept = [], []
            for r in range(a.repeat):
                # a new run each repeat: the held states start empty, as they do at the start of a sequence
                rh.set_particle_noise(a.noise_std if noisy else 0.0, a.noise_scale if noisy else 0.0, run_frame, run_seed)
                torch.cuda.synchronize()
                calls = []
                for b0 in range(0, n, B):
                    part = fr[b0:b0 + B]
                    t0 = time.perf_counter()
                    rh.generate_drops_device(part, H, W, drops.data_ptr(), cap, counts.data_ptr())
                    torch.cuda.synchronize()
                    calls.append(1e3 * (time.perf_counter() - t0))
                    kept.append(counts[:len(part)].cpu().numpy().mean())
                times.append(calls)
            best = min(times, key=sum)
            res['noise_on' if noisy else 'noise_off'] = dict(ms_total=round(sum(best), 3), ms_per_call=[round(v, 3) for v in best])
            res['drops_per_frame_mean'] = round(float(np.mean(kept)), 1)
        res['added_ms_per_call'] = round((res['noise_on']['ms_total'] - res['noise_off']['ms_total']) / len(best), 3)
        rh.close()
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
