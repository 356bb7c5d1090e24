"""Cost of the field particle model (rr_set_particle_model) against the default i.i.d. model: the particle kernel's own time
from the library profile (rr_profile_read: k_particles / k_field_particles, and k_particle_draws beside them) for
rr_generate_drops_device on one workload, both models in interleaved rounds inside one process, median / minimum / maximum
over the rounds.  The field model is timed for every --chunks value (RR_OPT_FIELD_CHUNKS: 0 = the library's choice, 1 = one
workgroup per frame, the shape of k_particles).  Prints one JSON line per batch size.

  python scripts/field_particle_cost.py [--workload nuscenes100] [--batches 8,32,512] [--rounds 7] [--calls 5] [--chunks 0,1]
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
    ap.add_argument('--workload', default='nuscenes100')
    ap.add_argument('--batches', default='8,32,512')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--chunks', default='0,1')
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
    wl = a.workload
    dataset, rate = wl.rstrip('0123456789'), int(wl[len(wl.rstrip('0123456789')):])
    opts = {k: v for k, v in db.settings(dataset).items() if k != 'sequences'}
    n_sim = particles.n_sim_frames(opts)
    W, H = (int(v) for v in opts['cam_CCD_WH'])
    chunk_opts = [int(c) for c in a.chunks.split(',')]
    runs = {}
    for model in ('iid', 'field'):
        sims, dgrid, cdf = particles.sim_frames(opts, rate, n_sim, seed=0, model=model)
        runs[model] = sims
    cap = int(runs['iid']['n_particles'].max() * 1.25)
    rh = hb.RainHip(0)
    rh.set_streak_db(streaks.streaks_light)
    rh.set_particle_tables(dgrid, cdf)
    legs = [('iid', 0)] + [('field', c) for c in chunk_opts]
    for B in (int(b) for b in a.batches.split(',')):
        drops = torch.empty((B, cap * hb.DROP_DTYPE.itemsize), dtype=torch.uint8, device='cuda:0')
        counts = torch.empty(B, dtype=torch.int32, device='cuda:0')
        f_idx = np.arange(B)
        frames = {'iid': runs['iid'][f_idx % n_sim].copy(), 'field': particles.field_run_sims(runs['field'], f_idx)}
        frames['iid']['draw_seed'] = f_idx
        per = {leg: dict(particles=[], draws=[]) for leg in legs}
        kept = {}

        def one(leg, timed):
            model, chunks = leg
            rh.set_particle_model(model, opts['cam_hz'])
            rh.set_option(hb.RR_OPT_FIELD_CHUNKS, chunks)
            rh.profile(True)
            rh.profile_reset()
            for _ in range(a.calls):
                rh.generate_drops_device(frames[model], H, W, drops.data_ptr(), cap, counts.data_ptr())
            torch.cuda.synchronize()
            st = rh.profile_read()
            rh.profile(False)
            kept[model] = float(counts.cpu().numpy().mean())
            if timed:
                name = 'k_particles' if model == 'iid' else 'k_field_particles'
                per[leg]['particles'].append(st[name][1] / a.calls)
                per[leg]['draws'].append(st['k_particle_draws'][1] / a.calls)
        for leg in legs:                                         # warm-up: every shape once
            one(leg, False)
        for _ in range(a.rounds):
            for leg in legs:
                one(leg, True)
        res = dict(workload=wl, frames_per_call=B, rounds=a.rounds, calls_per_round=a.calls, unit='ms per call',
                   kept_per_frame={m: round(v, 1) for m, v in kept.items()},
                   slots_per_frame=int(runs['field']['n_particles'].max()), particles_per_frame_iid=int(runs['iid']['n_particles'].max()))
        for (model, chunks), v in per.items():
            key = model if model == 'iid' else 'field_chunks%d' % chunks
            res[key] = dict(particle_kernel=_stats(v['particles']), k_particle_draws=_stats(v['draws']))
        for c in chunk_opts:
            res['field_chunks%d' % c]['ratio_to_iid_median'] = round(
                res['field_chunks%d' % c]['particle_kernel']['median'] / res['iid']['particle_kernel']['median'], 3)
        print(json.dumps(res), flush=True)
        del drops, counts
    rh.close()


if __name__ == '__main__':
    main()
