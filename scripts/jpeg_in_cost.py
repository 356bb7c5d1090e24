"""Cost of JPEG input frames (RR_IN_BG_JPEG): what the host / device split of the decoder costs and gains, three
measurements in one process on nuScenes-sized frames (--size, default 1600x900; 4:2:0 at quality 92, made from the synthetic scenes):

  host      CPU-ms per frame on ONE thread: rr_jpeg_read_record (markers + Huffman decoding, what the batch-native route leaves on the
            host), rr_jpeg_read_bgr8 (the whole decode on the host), PIL's full decode of the same file, and rr_io_read_frames_rows
            (inflate only) on the same pixels as a PNG file -- --files files, interleaved rounds;
  kernels   k_jpeg_idct and k_jpeg_bgr per batch of --batch frames beside k_png_unfilter<3> on the PNG form of the same pixels, from the
            library profile (HIP events around each launch, rr_profile_read);
  driver    main.py steady-state frames/s on a tree of --frames such frames: the general route with PIL's decoder (the only one before),
            the general route with the library's host decode, the batch-native JPEG route, and the PNG-rows route on converted files --
            --pairs interleaved rounds, batches of --driver-batch frames; the whole run (set-up of the first batch included) and the
            frames after the first batch.

Prints one JSON line; --md appends the same figures to a markdown file.  Informational: nothing is gated on the figures.

  python scripts/jpeg_in_cost.py [--size 1600x900] [--files 8] [--batch 64] [--rounds 5] [--frames 96] [--pairs 3] [--driver-batch 16] [--skip host,kernels,driver] [--md FILE]
"""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s):
    return '%.4g [%.4g .. %.4g]' % (s['median'], s['min'], s['max'])


def _files(tmp, n, W, H, synthetic):
    """n frames three ways: (jpg path, png path of PIL's decode of it, 16-bit depth png path)."""
    from PIL import Image
    out = []
    for i in range(n):
        rgb = (synthetic.make_frame(100 + i, H, W)[..., ::-1] * 255).astype(np.uint8)
        jp, pp, dp = (os.path.join(tmp, '%s%04d.%s' % (k, i, e)) for k, e in (('i', 'jpg'), ('p', 'png'), ('d', 'png')))
        Image.fromarray(rgb).save(jp, 'JPEG', quality=92, subsampling=2)
        Image.open(jp).convert('RGB').save(pp, compress_level=1)
        ramp = np.linspace(80.0, 2.0, H)[:, None] * np.ones((1, W))
        Image.fromarray(np.round(ramp * 256).astype(np.uint16)).save(dp)
        out.append((jp, pp, dp))
    return out


def host(a, hb, files, W, H):
    from PIL import Image
    import ctypes
    lib = hb.load_library()
    info = hb.jpeg_info(files[0][0])
    rb = hb.jpeg_record_bytes(info[1], info[2], info[4])
    rec = np.zeros(rb // 8, np.int64).view(np.uint8)
    px = np.empty((H, W, 3), np.uint8)
    rows_i = np.zeros((1, H * (1 + 3 * W)), np.uint8)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    cases = {
        'rr_jpeg_read_record': lambda f: lib.rr_jpeg_read_record(os.fsencode(f[0]), ptr(rec), rec.size),
        'rr_jpeg_read_bgr8': lambda f: lib.rr_jpeg_read_bgr8(os.fsencode(f[0]), ptr(px), H, W),
        'PIL full decode': lambda f: (np.array(Image.open(f[0]).convert('RGB')), 0)[1],
        'rr_io_read_frames_rows, image only (the same pixels as PNG)': lambda f: _rows_image(hb, f[1], H, W, rows_i),
    }
    t = {k: [] for k in cases}
    for rnd in range(a.rounds + 1):                                  # round 0: warm-up (file cache, buffer pools)
        for k, fn in cases.items():
            c0 = time.process_time()
            for f in files:
                assert fn(f) == 0, k
            if rnd:
                t[k].append((time.process_time() - c0) * 1e3 / len(files))
    return {k: _stats(v) for k, v in t.items()}, dict(jpg_bytes=int(np.mean([os.path.getsize(f[0]) for f in files])),
                                                       png_bytes=int(np.mean([os.path.getsize(f[1]) for f in files])), record_bytes=rb)


def _rows_image(hb, path, H, W, rows_i):
    import ctypes
    lib = hb.load_library()
    ip, keep = hb._c_paths([path])
    st = np.zeros(1, np.int32)
    rc = lib.rr_io_read_frames_rows(1, ip, None, H, W, rows_i.ctypes.data_as(ctypes.c_void_p), int(rows_i.strides[0]), None, 0, 1,
                                    st.ctypes.data_as(ctypes.c_void_p))
    return rc or int(st[0])


def kernels(a, hb, files, W, H):
    from PIL import Image
    fogmod = importlib.import_module('rain-rendering_amd.common.add_attenuation')
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from oracle import prepass as op
    rh = hb.RainHip(0)
    rh.set_prepass_kernels(op.gaussian_kernel(25, 25), op.gaussian_kernel(15, 0))
    consts = fogmod.FogRain(rain_intensity=25, focal=0.006, f_number=6.0, angle=90, exposure=2, camera_gain=20).constants()
    B = a.batch
    recs = [hb.jpeg_read_record(f[0]) for f in files]
    rows = [hb.png_rows_of(np.ascontiguousarray(np.array(Image.open(f[1]).convert('RGB'))[..., ::-1])) for f in files]
    depth = np.full((H, W), 20.0, np.float32)
    fj = [dict(bg_jpeg=recs[k % len(files)], shape=(H, W), depth=depth, fog=consts) for k in range(B)]
    fp = [dict(bg_png_rows=rows[k % len(files)], shape=(H, W), depth=depth, fog=consts) for k in range(B)]
    t = {'k_jpeg_idct': [], 'k_jpeg_bgr': [], 'k_png_unfilter': []}
    same = None
    for rnd in range(a.rounds + 1):
        for frames, names in ((fj, ('k_jpeg_idct', 'k_jpeg_bgr')), (fp, ('k_png_unfilter',))):
            rh.profile(True)
            rh.profile_reset()
            out = rh.prepass_frames(frames, want_env=False, out_dtype=np.float32)
            prof = rh.profile_read()
            rh.profile(False)
            for nm in names:
                assert prof[nm][0] == 1, (nm, prof.get(nm))
                if rnd:
                    t[nm].append(prof[nm][1])
            if rnd == 0:
                same = out if same is None else all(np.array_equal(x['rainy_bg'], y['rainy_bg']) for x, y in zip(same, out))
            del out
    rh.close()
    assert same is True, "the JPEG batch and the PNG batch of the same pixels gave different fog layers"
    return {k: _stats(v) for k, v in t.items()}


def driver(a, hb, W, H, synthetic):
    from PIL import Image
    main_mod = importlib.import_module('rain-rendering_amd.main')
    imgops = importlib.import_module('rain-rendering_amd.common.imgops')
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
        xml = os.path.join(tmp, 'particles', 'kitti', 'data_object', 'rain', '25mm', 'sim_camera0.xml')
        synthetic.write_particles_xml(xml, synthetic.simulate_particles(4, 400, W, H))
        trees = {}
        for kind in ('jpg', 'png'):
            src = os.path.join(tmp, 'source_' + kind)
            img_dir, _ = synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), a.frames, H, W, depth_m=None)
            for i in range(a.frames):
                png = os.path.join(img_dir, '%06d.png' % i)
                f = io.BytesIO()
                Image.open(png).convert('RGB').save(f, 'JPEG', quality=92, subsampling=2)
                if kind == 'jpg':
                    os.remove(png)
                    with open(os.path.join(img_dir, '%06d.jpg' % i), 'wb') as fh:
                        fh.write(f.getvalue())
                else:
                    Image.open(io.BytesIO(f.getvalue())).convert('RGB').save(png, compress_level=1)
            trees[kind] = src
        cases = (('general route, PIL decode (the route before)', 'jpg', '0', True), ('general route, library host decode', 'jpg', '0', False),
                 ('batch-native JPEG route', 'jpg', '1', False), ('batch-native PNG-rows route (converted files)', 'png', '1', False))
        t = {c[0]: [] for c in cases}
        t.update({c[0] + ', after the first batch': [] for c in cases})
        os.environ['RAIN_BATCH'] = str(a.driver_batch)
        native_jpeg = imgops._native_jpeg
        n_run = 0
        for rnd in range(a.pairs + 1):                               # round 0: warm-up
            for name, kind, native, pil in cases:
                os.environ['RAIN_NATIVE_IO'] = native
                imgops._native_jpeg = (lambda p: None) if pil else native_jpeg
                n_run += 1
                with contextlib.redirect_stdout(io.StringIO()):
                    gen = main_mod.main(['--dataset', 'kitti', '-k', trees[kind], '-d', trees[kind], '-r', os.path.join(tmp, 'particles'), '-sd',
                                         os.path.join(tmp, 'rainstreakdb'), '-i', '25', '--output', os.path.join(tmp, 'out%d' % n_run), '--noverbose'])
                imgops._native_jpeg = native_jpeg
                tm = gen.timing[0]
                assert tm['frames'] == a.frames and (tm.get('route') == 'native') == (native == '1'), (name, tm)
                if rnd:
                    t[name].append(tm['frames'] / tm['total_s'])
                    t[name + ', after the first batch'].append((tm['frames'] - a.driver_batch) / (tm['total_s'] - tm['first_batch_s']))
        os.environ.pop('RAIN_NATIVE_IO', None)
        os.environ.pop('RAIN_BATCH', None)
        for k, v in t.items():
            res[k] = _stats(v)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='1600x900')
    ap.add_argument('--files', type=int, default=8)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--driver-batch', type=int, default=16)
    ap.add_argument('--skip', default='')
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split('x'))
    skip = set(a.skip.split(','))
    import __graft_entry__ as ge
    ge.build()
    hb = importlib.import_module('rain-rendering_amd.hip_backend')
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    res = dict(metric='jpeg_in_cost', size=[W, H], files=a.files, batch=a.batch, rounds=a.rounds, frames=a.frames, pairs=a.pairs)
    with tempfile.TemporaryDirectory() as tmp:
        files = _files(tmp, a.files, W, H, synthetic)
        if 'host' not in skip:
            res['host_cpu_ms_per_frame'], res['bytes_per_frame'] = host(a, hb, files, W, H)
        if 'kernels' not in skip:
            res['kernel_ms_per_batch'] = kernels(a, hb, files, W, H)
    if 'driver' not in skip:
        res['driver_frames_per_s'] = driver(a, hb, W, H, synthetic)
    print(json.dumps(res))
    if a.md:
        with open(a.md, 'a') as fh:
            fh.write('\n`python scripts/jpeg_in_cost.py --size %s --files %d --batch %d --rounds %d --frames %d --pairs %d`, median [min .. max]:\n\n' % (
                a.size, a.files, a.batch, a.rounds, a.frames, a.pairs))
            for key, head in (('host_cpu_ms_per_frame', 'host, one thread | CPU-ms per frame'), ('kernel_ms_per_batch', 'kernel | ms per batch of %d' % a.batch),
                              ('driver_frames_per_s', 'main.py on %d frames, batches of %d | frames/s' % (a.frames, a.driver_batch))):
                if key in res:
                    fh.write('| %s |\n|---|---|\n' % head + ''.join('| %s | %s |\n' % (k, _cell(v)) for k, v in res[key].items()) + '\n')
            if 'bytes_per_frame' in res:
                fh.write('bytes per frame: %s\n' % json.dumps(res['bytes_per_frame']))


if __name__ == '__main__':
    main()
