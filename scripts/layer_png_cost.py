"""Cost of the rain layer as a file INSIDE the frame pipeline (rr_pipeline_set_layer_png): KITTI frames at 25 mm/hr in batches
of --pipe-batch through the three slots with the PNG payloads entropy-coded on the device (RR_OPT_PNG_DEFLATE), as the driver runs them.
Cases, in interleaved rounds inside one process:
  not armed                   two streams per frame
  float layer                 rr_pipeline_set_layer with a float32 [H, W, 4] buffer per frame: k_rain_layer<0>, 16 bytes per pixel
  layer file                  rr_pipeline_set_layer_png (and the shifts, as the driver arms it): k_rain_layer<2> storing 4 bytes per pixel,
                              k_png_layer, three streams
  layer file + float layer    the one walk stores both
  lens label                  rr_pipeline_set_lens with alpha_png: three streams, the extra one the label's
  lens label + layer file     four streams
Per case, from the library profile (rr_profile_read: HIP events on the compute stream), ms per batch of k_rain_layer, k_layer_finish,
k_png_layer and k_pngz (the codec) -- and, from a second pass WITHOUT the profile (its events serialise the slots), the pipeline's frames/s:
median [min .. max] over the rounds.  Prints one JSON line; --md appends the figures as table rows to a markdown file.  Informational.

  python scripts/layer_png_cost.py [--pipe-batch 64] [--rounds 5] [--batches 3] [--md FILE]
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
PARTS = ('k_rain_layer', 'k_layer_finish', 'k_png_layer', 'k_pngz')
CASES = (('not armed', False, False, False), ('float layer', True, False, False), ('layer file', False, True, False),
         ('layer file + float layer', True, True, False), ('lens label', False, False, True), ('lens label + layer file', False, True, True))


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s, fmt='%.3f'):
    return (fmt + ' [' + fmt + ' .. ' + fmt + ']') % (s['median'], s['min'], s['max'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pipe-batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', type=int, default=3, help='batches per round and case (a multiple of the three slots)')
    ap.add_argument('--lens-count', type=int, default=40)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    scenes = importlib.import_module('rain-rendering_amd.scenes')
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    lens = importlib.import_module('rain-rendering_amd.tools.lens')
    fogmod = importlib.import_module('rain-rendering_amd.common.add_attenuation')
    envmod = importlib.import_module('rain-rendering_amd.common.envmap')
    imgops = importlib.import_module('rain-rendering_amd.common.imgops')
    hb = scenes.hb
    H, W, RATE = 375, 1242, 25
    PB, nslot = a.pipe_batch, hb.RR_PIPE_SLOTS
    nd = min(PB, 16)                                   # distinct frames (the rest repeat them)
    sc = scenes.Scene(tempfile.mkdtemp(prefix='layerpng_'), H, W, synthetic.DROPS_PER_RATE[RATE], n_frames=nd, cam=scenes.KITTI)
    rh = hb.RainHip(0)
    rh.set_streak_db(sc.db.streaks_light)
    rh.set_camera(sc.cam)
    rh.set_colormap(imgops.viridis_lut())
    cs = sc.cam_settings
    consts = fogmod.FogRain(rain_intensity=RATE, focal=cs['focal_mm'] / 1000., f_number=cs['f_number'], angle=90, exposure=cs['exposure_ms'],
                            camera_gain=20).constants()
    rh.set_prepass_kernels(imgops.gaussian_kernel(25, 25), imgops.gaussian_kernel(15, 0))
    rh.set_envmap_geometry(H, W, *envmod.EnvironmentMapGenerator(cs['focal_mm'] / 1000., W, H).device_tables(H, W))
    rh.set_solid_angles(sc.omega)
    rh.set_option(hb.RR_OPT_PNG_DEFLATE, 1)
    depth = (np.linspace(80, 2, H, dtype=np.float32)[:, None] * np.ones((1, W), np.float32))
    host = [(sc.frame_inputs(i)[0], sc.product_drops(i)) for i in range(nd)]
    cap = (max(len(h_[1]) for h_ in host) + 3) // 4 * 4
    row = H * (1 + 4 * W)
    preps, labels, files, shifts, floats = [], [], [], [], []
    for s_ in range(nslot):
        arrs = [rh.host_rows(PB, shp, dt)[1] for shp, dt in (((H, W, 3), np.uint8), ((H, W), np.float32), ((cap,), hb.DROP_DTYPE),
                                                           ((cap,), np.int32), ((row,), np.uint8), ((row,), np.uint8), ((row,), np.uint8),
                                                           ((row,), np.uint8), ((1,), np.float64), ((H, W, 4), np.float32))]
        bg8s, deps, drs, sts, png_i, png_m, png_a, png_l, shift, lay = arrs
        frs, outs, nds = [], [], []
        for k in range(PB):
            bg, dr_ = host[(s_ * PB + k) % nd]
            bg8s[k][...] = (bg * 255).astype(np.uint8)
            deps[k][...] = depth
            drs[k][:len(dr_)] = dr_
            nds.append(len(dr_))
            frs.append(dict(bg_u8=bg8s[k], depth=deps[k], fog=consts, omega=None, drops=drs[k]))
            outs.append(dict(image_u8=None, rainy_png=png_i[k], mask_png=png_m[k], status=sts[k]))   # what the driver downloads
        prep = rh.pipeline_prepare(frs, outs)
        for k, n_ in enumerate(nds):
            prep.set_drop_count(k, n_)
        preps.append(prep)
        labels.append(png_a)
        files.append(png_l)
        shifts.append(shift)
        floats.append(lay)
    gen = lens.LensDrops(H, W, count=a.lens_count, seed=1)
    tabs = [[gen.table(7 * (s_ * PB + k)) for k in range(PB)] for s_ in range(nslot)]

    def arm(case):
        _, want_float, want_file, want_label = case
        for s_ in range(nslot):
            rh.pipeline_set_lens(s_, tabs[s_], gen.weights(), H, W, alpha_png=labels[s_]) if want_label else rh.pipeline_set_lens(s_, None)
            rh.pipeline_set_layer_png(s_, [files[s_][k] for k in range(PB)], H, W) if want_file else rh.pipeline_set_layer_png(s_, None)
            if want_float or want_file:                 # (the driver arms the shifts beside the file)
                rh.pipeline_set_layer(s_, [dict(layer=floats[s_][k] if want_float else None, shift=shifts[s_][k]) for k in range(PB)])
            else:
                rh.pipeline_set_layer(s_, None)

    def pipe(n_batches):
        t0 = time.perf_counter()
        for r in range(n_batches + nslot):
            s_ = r % nslot
            if r >= nslot:
                while not rh.pipeline_wait(s_):
                    rh.pipeline_submit_prepared(s_, preps[s_])
            if r < n_batches:
                rh.pipeline_submit_prepared(s_, preps[s_])
        return time.perf_counter() - t0

    per = {c[0]: dict({p: [] for p in PARTS}, fps=[]) for c in CASES}
    for case in CASES:                                  # warm-up: every case once (staging, arena, codec scratch)
        arm(case)
        pipe(nslot)
    for _ in range(a.rounds):
        for case in CASES:
            arm(case)
            rh.profile(True)
            rh.profile_reset()
            pipe(a.batches)
            st = rh.profile_read()
            rh.profile(False)
            for p in PARTS:
                per[case[0]][p].append(st.get(p, (0, 0.0))[1] / a.batches)
            per[case[0]]['fps'].append(a.batches * PB / pipe(a.batches))
    arm(CASES[0])
    rh.close()
    out = dict(workload='rr_pipeline_submit kitti %d mm/hr, %d frames per batch, three slots, RR_OPT_PNG_DEFLATE 1' % (RATE, PB), rounds=a.rounds,
               batches_per_round=a.batches, unit='ms per batch; frames/s', cases=[])
    rows = []
    for case in CASES:
        name = case[0]
        res = dict(case=name, streams=2 + int(case[2]) + int(case[3]), frames_per_s=_stats(per[name]['fps']))
        res.update({p: _stats(per[name][p]) for p in PARTS})
        out['cases'].append(res)
        rows.append('| %s | %d | %s | %s | %s | %s | %s |' % (name, res['streams'], _cell(res['k_rain_layer']), _cell(res['k_layer_finish']),
                                                            _cell(res['k_png_layer']), _cell(res['k_pngz']), _cell(res['frames_per_s'], '%.0f')))
    print(json.dumps(out), flush=True)
    if a.md:
        with open(a.md, 'a') as fh:
            fh.write('\n%s, %d rounds of %d batches: median [min .. max]\n\n' % (out['workload'], a.rounds, a.batches))
            fh.write('| case | streams | k_rain_layer ms | k_layer_finish ms | k_png_layer ms | k_pngz ms | pipeline frames/s |\n')
            fh.write('|---|---|---|---|---|---|---|\n')
            fh.write('\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
