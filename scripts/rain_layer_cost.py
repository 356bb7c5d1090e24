"""Cost of the rain layer (rr_pipeline_set_layer, k_rain_layer) on the benchmark's own step: --batch frames of a
bench.py workload resident in HBM through rr_render_frames_device, with slot 0 not armed and armed (layer [H, W, 4] float32 and
shift of every frame, device buffers), in interleaved rounds inside one process.  Per case the step time by a host clock
around --steps steps that end in rr_synchronize, median [min .. max] over the rounds, and from a second pass with the library profile (rr_profile_read: HIP
events around every launch, which serialise the two streams) k_rain_layer's, k_layer_finish's and the compositor's own time per
step.  Prints one JSON line; --md appends the figures to a markdown file.  Informational: the layer has no target; what is
required is that the step that is not armed does not slow (profiles/rain_layer_cost.md).

  python scripts/rain_layer_cost.py [--workload kitti100] [--batch 512] [--rounds 7] [--steps 3] [--md FILE]
"""
import argparse
import contextlib
import ctypes
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCOPES = ('k_rain_layer', 'k_layer_finish', 'k_composite')


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s):
    return '%.3f [%.3f .. %.3f]' % (s['median'], s['min'], s['max'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='kitti100')
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    import bench
    wl = bench.WORKLOADS[a.workload]
    assert not wl.get('sim'), 'a workload with drop tables from the host'
    scenes = importlib.import_module('rain-rendering_amd.scenes')
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    hb = scenes.hb
    H, W, B = wl['H'], wl['W'], a.batch
    cam = getattr(scenes, wl['cam'])
    simulated = bench.start_simulation(B, synthetic.DROPS_PER_RATE[wl['rate']], W, H, cam, 3000, wl['rs'], max(1, min(16, os.cpu_count() or 1)))
    import torch
    if not torch.cuda.is_available():
        simulated(cancel=True)
        raise SystemExit("rain_layer_cost.py needs a GPU: the hot path has no CPU fallback")
    import __graft_entry__ as ge
    ge.build()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    with contextlib.redirect_stdout(sys.stderr):
        sc = bench.lean_scene(scenes, tempfile.mkdtemp(prefix='layercost_'), H, W, cam, wl['rs'], simulated())
    rh = hb.RainHip(0)
    texels, hs, ws, offs = hb.pack_streak_db(sc.db.streaks_light)
    t_tex = torch.from_numpy(texels).to(dev)
    rh.set_streak_db_device(t_tex.data_ptr(), t_tex.numel(), hs, ws, offs)
    rh.set_camera(sc.cam)
    batch = bench.DeviceBatch(torch, hb, sc, dev, list(range(B)), list(range(B)))
    stream = torch.cuda.current_stream().cuda_stream
    layer = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    shift = torch.empty((B,), dtype=torch.float64, device=dev)
    tab = (hb.rr_layer_out * B)()
    for f in range(B):
        tab[f].layer, tab[f].shift = layer[f].data_ptr(), shift[f:f + 1].data_ptr()
    armed = hb.rr_pipeline_layer()
    armed.n, armed.frames = B, ctypes.cast(tab, ctypes.c_void_p)

    def arm(on):
        rh._check(rh.lib.rr_pipeline_set_layer(rh.h, 0, ctypes.byref(armed) if on else None), 'rr_pipeline_set_layer')

    def step():
        rh.render_frames_device(batch.fin, batch.fout, B, stream)

    def steps_ms():
        torch.cuda.synchronize()                         # host clock around steps that end in the library's own synchronise
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        assert rh.synchronize(), 'the arena regrew inside a timed round'
        return 1e3 * (time.perf_counter() - t0) / a.steps

    for on in (False, True):                            # warm-up: sizes the arena, the scratch and the descriptor rings
        arm(on)
        for _ in range(2):
            step()
            while not rh.synchronize():
                step()
    per = {on: dict(step=[], **{s: [] for s in SCOPES}) for on in (False, True)}
    for _ in range(a.rounds):
        for on in (False, True):
            arm(on)
            per[on]['step'].append(steps_ms())
            rh.profile_reset()
            rh.profile(True)
            for _k in range(a.steps):
                step()
            assert rh.synchronize(), 'the arena regrew inside a timed round'
            rh.profile(False)
            st = rh.profile_read()
            for s in SCOPES:
                per[on][s].append(st.get(s, (0, 0.0))[1] / a.steps)
    arm(False)
    dry = float((layer[..., 3] == 1).float().mean())
    rh.close()
    out = dict(workload='%s, %d frames per step, rr_render_frames_device' % (a.workload, B), rounds=a.rounds, steps_per_round=a.steps, unit='ms per step',
               layer_bytes_per_step=int(B) * H * W * 16, share_of_pixels_without_rain=round(dry, 4),
               not_armed={k: _stats(v) for k, v in per[False].items()}, armed={k: _stats(v) for k, v in per[True].items()})
    print(json.dumps(out))
    if a.md:
        with open(a.md, 'a') as f:
            f.write('\n| case | step | k_composite | k_rain_layer | k_layer_finish |\n|---|---|---|---|---|\n')
            for name, on in (('not armed', False), ('armed', True)):
                f.write('| %s | %s | %s | %s | %s |\n' % ((name, _cell(out['armed' if on else 'not_armed']['step'])) +
                                                        tuple(_cell(out['armed' if on else 'not_armed'][s]) for s in ('k_composite', 'k_rain_layer', 'k_layer_finish'))))


if __name__ == '__main__':
    main()
