"""Cost of the render-scale resize on the device (rr_set_input_resize), two measurements in one process:

  kernels   k_resize_in / k_resize_depth per frame, from the library profile (HIP events around each launch, rr_profile_read):
            --size render frames from files of twice the size (default 1024x512 <- 2048x1024: Cityscapes at render_scale 2), batch
            --batch, the three image kinds and both depth kinds, warmed up, median [min .. max] over --rounds calls;
  driver    main.py steady-state frames/s on a synthetic Cityscapes-shaped tree (synthetic.write_dataset: files of twice the render
            size, depth files of the render size, render_scale 2 / depth_scale 2, --frames frames) with and without --device_resize:
            --pairs alternating pairs of runs, medians and spread, beside the bytes each route uploads per frame (from the shapes).

Prints one JSON line; --md appends the same figures to a markdown file.  Informational: nothing is gated on the figures.

  python scripts/input_resize_cost.py [--size 1024x512] [--batch 32] [--rounds 9] [--frames 512] [--pairs 5] [--rate 25] [--md FILE]
"""
import argparse
import contextlib
import importlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s):
    return '%.4g [%.4g .. %.4g]' % (s['median'], s['min'], s['max'])


def kernels(a, torch, hb, W, H):
    """us per frame of each kernel kind at batch a.batch."""
    dev = torch.device('cuda', 0)
    hip = hb.RainHip(0)
    sh, sw, B = 2 * H, 2 * W, a.batch
    g = torch.Generator(device='cpu').manual_seed(1)
    u8 = torch.randint(0, 256, (B, sh, sw, 3), dtype=torch.uint8, generator=g)
    inputs = {'bgr_u8': (u8.to(dev), hb.RR_RESIZE_BGR_U8), 'rgb_u8_planar': (u8.permute(0, 3, 1, 2).contiguous().to(dev), hb.RR_RESIZE_RGB_U8_PLANAR),
              'rgb_f32_planar': ((u8.permute(0, 3, 1, 2).contiguous().float() / 255.0).to(dev), hb.RR_RESIZE_RGB_F32_PLANAR)}
    d16 = torch.randint(512, 20480, (B, sh, sw), dtype=torch.int32, generator=g)
    depths = {'u16': (d16.to(torch.int16).to(dev), hb.RR_DEPTH_U16), 'f32': ((d16.float() / 256.0).to(dev), 0)}
    bg = torch.empty((B, H, W, 3), dtype=torch.float64, device=dev)
    dep = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    hip.set_input_resize(sh, sw, sh, sw)
    out = {}

    def call(img, ik, d, dk):
        hip._check(hip.lib.rr_resize_inputs_device(hip.h, B, H, W, img.data_ptr() if img is not None else None, ik, d.data_ptr() if d is not None else None, dk,
                                                   bg.data_ptr() if img is not None else None, dep.data_ptr() if d is not None else None, None),
                   'rr_resize_inputs_device')
    for scope, cases in (('k_resize_in', inputs), ('k_resize_depth', depths)):
        for name, (t, kind) in cases.items():
            args = (t, kind, None, 0) if scope == 'k_resize_in' else (None, 0, t, kind)
            for _ in range(3):
                call(*args)
            per = []
            for _ in range(a.rounds):
                hip.profile(True)
                hip.profile_reset()
                call(*args)
                st = hip.profile_read()
                hip.profile(False)
                per.append(1e3 * st[scope][1] / st[scope][0] / B)
            src_b = t.numel() * t.element_size() / B
            dst_b = H * W * (24 if scope == 'k_resize_in' else 4)
            s = _stats(per)
            out['%s %s' % (scope, name)] = dict(us_per_frame=s, bytes_read_per_frame=int(src_b), bytes_written_per_frame=dst_b,
                                                gb_per_s=round((src_b + dst_b) / (s['median'] * 1e-6) / 1e9, 1))
    hip.close()
    return out


def driver(a, W, H):
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    main_mod = importlib.import_module('rain-rendering_amd.main')
    kitti = importlib.import_module('rain-rendering_amd.config.kitti')
    plain = kitti.settings
    sh, sw = 2 * H, 2 * W

    def scaled():                                        # the Cityscapes plug-in's scales on the tree layout write_dataset makes
        st = dict(plain())
        st.update(render_scale=2, depth_scale=2, cam_WH=[sw, sh], cam_CCD_WH=[sw, sh])
        return st
    kitti.settings = scaled
    os.environ['RAIN_BATCH'] = str(a.batch)
    fps = {'default': [], 'device_resize': []}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            from PIL import Image
            src = os.path.join(tmp, 'source')
            nd = min(a.distinct, a.frames)
            img_dir, dep_dir = synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), nd, sh, sw, depth_m=None)
            for i in range(nd):                              # depth files of the render size (depth_scale 2)
                ramp = np.linspace(80.0, 2.0, H)[:, None] * np.ones((1, W)) + (i % 7)
                Image.fromarray(np.round(ramp * 256).astype(np.uint16)).save(os.path.join(dep_dir, '%06d.png' % i))
            for i in range(nd, a.frames):
                os.symlink(os.path.join(img_dir, '%06d.png' % (i % nd)), os.path.join(img_dir, '%06d.png' % i))
                os.symlink(os.path.join(dep_dir, '%06d.png' % (i % nd)), os.path.join(dep_dir, '%06d.png' % i))
            synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
            xml = os.path.join(tmp, 'particles', 'kitti', 'data_object', 'rain', '%dmm' % a.rate, 'sim_camera0.xml')
            synthetic.write_particles_xml(xml, synthetic.simulate_particles(4, synthetic.DROPS_PER_RATE[a.rate], sw, sh))
            for pair in range(a.pairs + 1):                  # pair 0 warms both routes up (page-locking, first-use allocations)
                for name in ('default', 'device_resize'):
                    out = os.path.join(tmp, 'out_%s_%d' % (name, pair))
                    argv = ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', os.path.join(tmp, 'rainstreakdb'),
                            '-i', str(a.rate), '--output', out, '--noverbose'] + (['--device_resize'] if name == 'device_resize' else [])
                    with contextlib.redirect_stdout(sys.stderr):         # (the driver's progress lines: this script prints one JSON line)
                        gen = main_mod.main(argv)
                    assert len(gen.stats) == a.frames and gen.timing[0]['route'] == 'native', gen.timing
                    if pair:
                        fps[name].append(gen.timing[0]['steady_frames_per_s'])
                    shutil.rmtree(out, ignore_errors=True)
    finally:
        kitti.settings = plain
    return dict(frames=a.frames, batch=a.batch, pairs=a.pairs, cpu_quota=importlib.import_module('rain-rendering_amd.common.generator')._cpu_budget(),
                steady_frames_per_s={k: _stats(v) for k, v in fps.items()},
                upload_bytes_per_frame={'default': H * W * 24 + H * W * 4, 'device_resize': sh * (1 + 3 * sw) + H * (1 + 2 * W)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='1024x512', help='render size W x H; the files are twice as large')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--frames', type=int, default=512)
    ap.add_argument('--distinct', type=int, default=32, help='distinct image / depth files; the rest of the sequence links to them')
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--rate', type=int, default=25)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    import torch                                         # (before the library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    hb = importlib.import_module('rain-rendering_amd.hip_backend')
    W, H = [int(v) for v in a.size.split('x')]
    out = dict(what='input resize on the device: %dx%d <- %dx%d' % (W, H, 2 * W, 2 * H), kernels=kernels(a, torch, hb, W, H))
    if a.frames > 0:
        out['driver'] = driver(a, W, H)
    print(json.dumps(out), flush=True)
    if a.md:
        with open(a.md, 'a') as fh:
            fh.write('\n%s, batch %d, us per frame: median [min .. max] of %d calls\n\n' % (out['what'], a.batch, a.rounds))
            fh.write('| kernel, input | us per frame | bytes read | bytes written | GB/s |\n|---|---|---|---|---|\n')
            for k, v in out['kernels'].items():
                fh.write('| %s | %s | %d | %d | %.1f |\n' % (k, _cell(v['us_per_frame']), v['bytes_read_per_frame'], v['bytes_written_per_frame'], v['gb_per_s']))
            if 'driver' in out:
                d = out['driver']
                fh.write('\nmain.py, %d frames, batch %d, CPU quota %s, steady-state frames/s: median [min .. max] of %d alternating pairs\n\n' %
                         (d['frames'], d['batch'], d['cpu_quota'], d['pairs']))
                fh.write('| route | frames/s | bytes uploaded per frame |\n|---|---|---|\n')
                for k in ('default', 'device_resize'):
                    fh.write('| %s | %s | %d |\n' % (k, _cell(d['steady_frames_per_s'][k]), d['upload_bytes_per_frame'][k]))


if __name__ == '__main__':
    main()
