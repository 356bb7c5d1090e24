"""Cost of a rate series (rr_set_particle_rate_series): the PARTICLE STEP of rr_generate_drops_device -- the particle kernel
(k_field_particles / k_rig_particles; count pass included where the batch is small) plus k_particle_draws where it is launched --
from the library profile (rr_profile_read), with no series, a series that sits at its peak (the same records: what the look-up and
the decision cost) and a ramp from the peak down to --low of it over the call's time indices (fewer records: what the thinning
saves) in interleaved rounds inside one process, median [min .. max] over the rounds.  The field model at --batches frames per call,
the rig model (stereo) at --instants instants per call, under --draws.  Prints one JSON line per model, draw mode and batch size;
--md appends the same figures as table rows to a markdown file.  Informational: the series has no target, only the ratio to none.

  python scripts/showers_cost.py [--workload kitti25] [--low 0.2] [--models field] [--draws counter] [--batches 32,512]
                                 [--instants 16,256] [--rounds 7] [--calls 5] [--md FILE]
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
KERNEL = {'field': 'k_field_particles', 'rig': 'k_rig_particles'}
MODES = ('off', 'peak', 'ramp')


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s):
    return '%.3f [%.3f .. %.3f]' % (s['median'], s['min'], s['max'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='kitti25')
    ap.add_argument('--low', type=float, default=0.2)
    ap.add_argument('--models', default='field')
    ap.add_argument('--draws', default='counter')
    ap.add_argument('--batches', default='32,512')
    ap.add_argument('--instants', default='16,256')
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
    s_field, dgrid, cdf_field = particles.sim_frames(opts, rate, 1, seed=0, model='field')
    s_rig, _, cdf_rig = particles.sim_frames(opts, rate, 1, seed=0, model='rig', rig=rig)
    tabs = [np.atleast_2d(cdf_field), np.atleast_2d(cdf_rig)]                                  # one context, every table
    s_rig['table'] += len(tabs[0])
    cap = int(s_field['n_particles'].max() / 2)
    rh = hb.RainHip(0)
    rh.set_streak_db(streaks.streaks_light)
    rh.set_particle_tables(dgrid, np.concatenate(tabs))
    rh.set_particle_rig(rig.as_records(), rig.box(particles.FrameCamera(opts, 0)))
    rows = []
    shapes = [(m, int(b)) for m in a.models.split(',') if m for b in a.batches.split(',')] + [('rig', int(b)) for b in a.instants.split(',')]
    for draws in a.draws.split(','):
        for model, n in shapes:
            B = n * V if model == 'rig' else n
            drops = torch.empty((B, cap * hb.DROP_DTYPE.itemsize), dtype=torch.uint8, device='cuda:0')
            counts = torch.empty(B, dtype=torch.int32, device='cuda:0')
            idx = np.arange(n)
            if model == 'field':
                frames = particles.field_run_sims(s_field, idx)
            else:
                frames = particles.rig_run_sims(s_rig, idx, V)
            rh.set_particle_model(model, opts['cam_hz'])
            rh.set_particle_draws(draws)
            series = dict(off=None, peak=particles.RateSeries(0, [float(rate)] * (n + 1)),      # cover the call's time indices 0 .. n - 1
                          ramp=particles.RateSeries(0, np.linspace(float(rate), a.low * float(rate), n + 1)))
            per = {j: dict(kernel=[], step=[]) for j in MODES}
            kept, small = {}, {}

            def one(j, timed):
                rh.set_particle_rate_series(series[j])
                rh.profile(True)
                rh.profile_reset()
                for _ in range(a.calls):
                    rh.generate_drops_device(frames, H, W, drops.data_ptr(), cap, counts.data_ptr())
                torch.cuda.synchronize()
                st = rh.profile_read()
                rh.profile(False)
                kept[j] = float(counts.cpu().numpy().mean())
                if timed:
                    k = st[KERNEL[model]][1] / a.calls
                    per[j]['kernel'].append(k)
                    per[j]['step'].append(k + st.get('k_particle_draws', (0, 0.0))[1] / a.calls)
            for j in per:                                            # warm-up: both shapes once
                one(j, False)
            for _ in range(a.rounds):
                for j in per:
                    one(j, True)
            rh.set_particle_rate_series(None)
            res = dict(workload=wl, model=model, draws=draws, ramp_low=a.low, frames_per_call=B, rounds=a.rounds, calls_per_round=a.calls,
                       unit='ms per call', kept_per_frame=round(kept['off'], 1), kept_per_frame_peak=round(kept['peak'], 1),
                       kept_per_frame_ramp=round(kept['ramp'], 1), candidates_per_frame=int(frames['n_particles'][0]))
            if model == 'rig':
                res.update(rig=a.rig, instants=n)
            for j, v in per.items():
                res[j] = dict(particle_kernel=_stats(v['kernel']), particle_step=_stats(v['step']))
            res['kernel_peak_over_off'] = round(res['peak']['particle_kernel']['median'] / res['off']['particle_kernel']['median'], 3)
            res['kernel_ramp_over_off'] = round(res['ramp']['particle_kernel']['median'] / res['off']['particle_kernel']['median'], 3)
            res['step_ramp_over_off'] = round(res['ramp']['particle_step']['median'] / res['off']['particle_step']['median'], 3)
            print(json.dumps(res), flush=True)
            rows.append('| %s | %s | %d | %.0f / %.0f / %.0f | %s | %s | %s | %.3f | %.3f | %.3f |' % (
                model, draws, B, res['kept_per_frame'], res['kept_per_frame_peak'], res['kept_per_frame_ramp'], _cell(res['off']['particle_kernel']),
                _cell(res['peak']['particle_kernel']), _cell(res['ramp']['particle_kernel']), res['kernel_peak_over_off'],
                res['kernel_ramp_over_off'], res['step_ramp_over_off']))
            del drops, counts
    rh.close()
    if a.md:
        with open(a.md, 'a') as fh:
            fh.write('\n%s, ramp to %g of the peak, %d rounds of %d calls, ms per call: median [min .. max]\n\n' % (wl, a.low, a.rounds, a.calls))
            fh.write('| model | draws | frames per call | kept per frame: no series / at the peak / ramp | particle kernel, no series | '
                     'particle kernel, series at its peak | particle kernel, ramp | peak / none | ramp / none | particle step, ramp / none |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|---|\n')
            fh.write('\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
