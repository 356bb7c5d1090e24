"""Cost of the two per-drop draw modes (rr_set_particle_draws): the PARTICLE STEP of rr_generate_drops_device -- the particle kernel
(k_particles / k_field_particles / k_rig_particles) plus k_particle_draws where it is launched -- from the library profile
(rr_profile_read), under RR_DRAWS_STREAM and RR_DRAWS_COUNTER in interleaved rounds inside one process, median [min .. max] over
the rounds.  The i.i.d. and field models at --batches frames per call, the rig model (stereo) at --instants instants per call.
Prints one JSON line per model and batch size; --md appends the same figures as table rows to a markdown file.

  python scripts/draws_cost.py [--workload kitti25] [--batches 8,32,128,512] [--instants 8,32,128] [--rounds 7] [--calls 5] [--md FILE]
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
KERNEL = {'iid': 'k_particles', 'field': 'k_field_particles', 'rig': 'k_rig_particles'}


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s):
    return '%.3f [%.3f .. %.3f]' % (s['median'], s['min'], s['max'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='kitti25')
    ap.add_argument('--batches', default='8,32,128,512')
    ap.add_argument('--instants', default='8,32,128')
    ap.add_argument('--rig', default='stereo:0.54')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--md', default=None)
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
    n_sim = particles.n_sim_frames(opts)
    W, H = (int(v) for v in opts['cam_CCD_WH'])
    rig = rigmod.Rig.from_spec(a.rig)
    V = len(rig)
    s_iid, dgrid, cdf_iid = particles.sim_frames(opts, rate, n_sim, seed=0)
    s_field, _, cdf_field = particles.sim_frames(opts, rate, 1, seed=0, model='field')
    s_rig, _, cdf_rig = particles.sim_frames(opts, rate, 1, seed=0, model='rig', rig=rig)
    tabs = [np.atleast_2d(cdf_iid), np.atleast_2d(cdf_field), np.atleast_2d(cdf_rig)]           # one context, every table
    s_field['table'] += len(tabs[0])
    s_rig['table'] += len(tabs[0]) + len(tabs[1])
    cap = int(max(s_iid['n_particles'].max() * 1.25, s_field['n_particles'].max() / 2))
    rh = hb.RainHip(0)
    rh.set_streak_db(streaks.streaks_light)
    rh.set_particle_tables(dgrid, np.concatenate(tabs))
    rh.set_particle_rig(rig.as_records(), rig.box(particles.FrameCamera(opts, 0)))
    rows = []
    shapes = [(m, int(b)) for m in ('iid', 'field') for b in a.batches.split(',')] + [('rig', int(b)) for b in a.instants.split(',')]
    for model, n in shapes:
        B = n * V if model == 'rig' else n
        drops = torch.empty((B, cap * hb.DROP_DTYPE.itemsize), dtype=torch.uint8, device='cuda:0')
        counts = torch.empty(B, dtype=torch.int32, device='cuda:0')
        idx = np.arange(n)
        if model == 'iid':
            frames = s_iid[idx % n_sim].copy()
            frames['draw_seed'] = idx
        elif model == 'field':
            frames = particles.field_run_sims(s_field, idx)
        else:
            frames = particles.rig_run_sims(s_rig, idx, V)
        rh.set_particle_model(model, opts['cam_hz'])
        per = {d: dict(kernel=[], draws=[], step=[]) for d in ('stream', 'counter')}
        kept = {}

        def one(draws, timed):
            rh.set_particle_draws(draws)
            rh.profile(True)
            rh.profile_reset()
            for _ in range(a.calls):
                rh.generate_drops_device(frames, H, W, drops.data_ptr(), cap, counts.data_ptr())
            torch.cuda.synchronize()
            st = rh.profile_read()
            rh.profile(False)
            kept[draws] = float(counts.cpu().numpy().mean())
            if timed:
                k = st[KERNEL[model]][1] / a.calls
                d = st.get('k_particle_draws', (0, 0.0))[1] / a.calls
                per[draws]['kernel'].append(k)
                per[draws]['draws'].append(d)
                per[draws]['step'].append(k + d)
        for d in per:                                            # warm-up: both shapes once
            one(d, False)
        for _ in range(a.rounds):
            for d in per:
                one(d, True)
        rh.set_particle_draws('stream')
        assert kept['stream'] == kept['counter']
        res = dict(workload=wl, model=model, frames_per_call=B, rounds=a.rounds, calls_per_round=a.calls, unit='ms per call',
                   kept_per_frame=round(kept['stream'], 1))
        if model == 'rig':
            res.update(rig=a.rig, instants=n)
        for d, v in per.items():
            res[d] = dict(particle_kernel=_stats(v['kernel']), k_particle_draws=_stats(v['draws']), particle_step=_stats(v['step']))
        res['counter_kernel_over_stream_kernel'] = round(res['counter']['particle_kernel']['median'] / res['stream']['particle_kernel']['median'], 3)
        res['stream_step_over_counter_step'] = round(res['stream']['particle_step']['median'] / res['counter']['particle_step']['median'], 2)
        print(json.dumps(res), flush=True)
        rows.append('| %s | %d | %s | %s | %s | %s | %.3f | %.2f |' % (
            model, B, _cell(res['stream']['particle_kernel']), _cell(res['stream']['k_particle_draws']),
            _cell(res['counter']['particle_kernel']), _cell(res['counter']['particle_step']),
            res['counter_kernel_over_stream_kernel'], res['stream_step_over_counter_step']))
        del drops, counts
    rh.close()
    if a.md:
        with open(a.md, 'a') as fh:
            fh.write('\n%s, %d rounds of %d calls, ms per call: median [min .. max]\n\n' % (wl, a.rounds, a.calls))
            fh.write('| model | frames per call | stream: particle kernel | stream: k_particle_draws | counter: particle kernel | '
                     'counter: particle step | counter kernel / stream kernel | stream step / counter step |\n')
            fh.write('|---|---|---|---|---|---|---|---|\n')
            fh.write('\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
