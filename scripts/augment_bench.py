"""RainAugment throughput (rain-rendering_amd/augment.py): one JSON line.

frames/s of a whole call at B = 8, 32, 128 KITTI-sized frames (1242 x 375) at 25 mm/hr for uint8 and float32 batches, the time
of the two tensor-layout kernels (k_planar_in, k_finalize_planar) per frame from rr_profile_read, and the host time per call
spent outside the GPU (input checks, record building, descriptor).  Synthetic streak database and images.  --draws counter times
RainAugment(draws='counter') (the texture pick from the drop's own counter: no k_particle_draws pass) in every leg; --jitter DEG
times RainAugment(jitter=DEG) (the per-drop streak jitter, made by the particle kernels)."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='8,32,128')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--intensity', type=float, default=25.0)
    ap.add_argument('--compare_models', type=int, default=0, metavar='ROUNDS',
                    help="also time particle_model 'iid' against 'field' at B = 32 (uint8) in this many interleaved rounds of --steps "
                         "calls; adds the key particle_models (frames/s: median, min, max over the rounds)")
    ap.add_argument('--rig', default=None, metavar='SPEC',
                    help="also time RainAugment(particle_model='rig') for this rig ('stereo:0.54' or a JSON file) at 32 frames per call "
                         "(uint8, 32 / V instants); adds the key rig (frames/s over --steps calls)")
    ap.add_argument('--draws', default='stream', choices=['stream', 'counter'], help="RainAugment(draws=...) of every leg")
    ap.add_argument('--jitter', type=float, default=0.0, metavar='DEG', help="RainAugment(jitter=...) of every leg (0: off)")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    augment = importlib.import_module('rain-rendering_amd.augment')
    dev = torch.device('cuda', 0)
    out = dict(workload='RainAugment kitti %g mm/hr' % args.intensity, draws=args.draws, jitter=args.jitter, steps=args.steps, fps={}, kernel_ms_per_frame={},
               host_ms_per_call={})
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, 'rainstreakdb')
        synthetic.write_streak_db(db)
        aug = augment.RainAugment('kitti', streaks_db=db, sequence='data_object/training', draws=args.draws, jitter=args.jitter)
        H, W = aug.frame_size()
        Bmax = max(int(b) for b in args.batches.split(','))
        base = np.stack([(synthetic.make_frame(i, H, W)[..., ::-1] * 255).astype(np.uint8) for i in range(8)])
        img8 = torch.from_numpy(np.ascontiguousarray(base.transpose(0, 3, 1, 2))).to(dev)
        img8 = img8.repeat((Bmax + 7) // 8, 1, 1, 1)[:Bmax].contiguous()
        depth = (torch.linspace(80.0, 2.0, H, device=dev)[:, None] * torch.ones((1, W), device=dev)).expand(Bmax, H, W).contiguous()
        rng = np.random.RandomState(0)
        for dt in ('uint8', 'float32'):
            img = img8 if dt == 'uint8' else (img8.float() / 255.0)
            for B in (int(b) for b in args.batches.split(',')):
                x, d = img[:B], depth[:B]
                for _ in range(args.warmup):
                    aug(x, d, args.intensity, rng.randint(0, 1 << 20, B))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    aug(x, d, args.intensity, rng.randint(0, 1 << 20, B))
                torch.cuda.synchronize()
                out['fps']['%s_B%d' % (dt, B)] = round(B * args.steps / (time.perf_counter() - t0), 1)
            # kernel times at B = 32 (or the largest batch below it)
            B = min(32, Bmax)
            hip = aug._hip
            hip.profile(True)
            hip.profile_reset()
            for _ in range(args.steps):
                aug(img[:B], depth[:B], args.intensity, rng.randint(0, 1 << 20, B))
            stats = hip.profile_read()
            hip.profile(False)
            for k in ('k_planar_in', 'k_finalize_planar'):
                launches, ms = stats.get(k, (0, 0.0))
                out['kernel_ms_per_frame']['%s_%s' % (dt, k)] = round(ms / max(B * args.steps, 1), 5)
            # host side of a call: input checks + records + descriptor (what runs before the library call)
            for Bh in (int(b) for b in args.batches.split(',')):
                x = img[:Bh]
                t0 = time.perf_counter()
                for _ in range(20):
                    aug._validate(x, depth[:Bh])
                    aug.plan(args.intensity, rng.randint(0, 1 << 20, Bh), Bh)
                out['host_ms_per_call']['%s_B%d' % (dt, Bh)] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
        aug.close()
        if args.compare_models > 0:
            B = min(32, Bmax)
            augs = {m: augment.RainAugment('kitti', streaks_db=db, sequence='data_object/training', particle_model=m, draws=args.draws, jitter=args.jitter) for m in ('iid', 'field')}
            rates = {m: [] for m in augs}
            k0 = 0
            for r in range(args.warmup + args.compare_models):
                for m, a in augs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s_ in range(args.steps):              # clips: consecutive indices, the same ones for both models
                        a(img8[:B], depth[:B], args.intensity, k0 + s_ * B + np.arange(B))
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        rates[m].append(B * args.steps / (time.perf_counter() - t0))
                k0 += args.steps * B
            out['particle_models'] = dict(B=B, rounds=args.compare_models, fps={
                m: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1)) for m, v in rates.items()})
            for a in augs.values():
                a.close()
        if args.rig:
            rig = importlib.import_module('rain-rendering_amd.rig').Rig.from_spec(args.rig)
            V = len(rig)
            Bi = max(min(32, Bmax) // V, 1)
            a = augment.RainAugment('kitti', streaks_db=db, sequence='data_object/training', particle_model='rig', rig=rig, draws=args.draws, jitter=args.jitter)
            x = img8[:Bi * V].reshape(Bi, V, 3, H, W)
            d = depth[:Bi * V].reshape(Bi, V, H, W)
            for r in range(args.warmup + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s_ in range(args.steps):
                    a(x, d, args.intensity, r * args.steps * Bi + s_ * Bi + np.arange(Bi))
                torch.cuda.synchronize()
                dt_ = time.perf_counter() - t0
            out['rig'] = dict(spec=args.rig, views=V, instants_per_call=Bi, frames_per_call=Bi * V, fps=round(Bi * V * args.steps / dt_, 1))
            a.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
