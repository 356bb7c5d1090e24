"""Cost of the drops on the lens (rr_lens_drops_device behind RainAugment(lens=)): the LENS PASS per call -- the device-to-device copy
(lens_copy) and k_lens_drops; the upload kernel is not clocked, like the library's other uploads -- from the library profile (rr_profile_read), beside
the RAIN STEP of the same call (every other profiled kernel of rr_augment_frames_device), at --batches KITTI-sized frames per call,
bytes and float32, with --counts drops on the lens, in interleaved rounds inside one process: median [min .. max] over the rounds.
Prints one JSON line; --md appends the same figures as table rows to a markdown file.  Informational: the pass has no target.

  python scripts/lens_cost.py [--batches 8,32,128] [--counts 40,128] [--rounds 5] [--calls 3] [--intensity 25] [--md FILE]
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
LENS = ('lens_copy', 'k_lens_drops')


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s):
    return '%.3f [%.3f .. %.3f]' % (s['median'], s['min'], s['max'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='8,32,128')
    ap.add_argument('--counts', default='40,128')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--intensity', type=float, default=25.0)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    augment = importlib.import_module('rain-rendering_amd.augment')
    lens = importlib.import_module('rain-rendering_amd.tools.lens')
    dev = torch.device('cuda', 0)
    batches = [int(b) for b in a.batches.split(',')]
    counts = [int(c) for c in a.counts.split(',')]
    out = dict(workload='RainAugment(lens=) kitti %g mm/hr' % a.intensity, rounds=a.rounds, calls_per_round=a.calls, unit='ms per call', cases=[])
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, 'rainstreakdb')
        synthetic.write_streak_db(db)
        kw = dict(streaks_db=db, sequence='data_object/training')
        H, W = augment.RainAugment('kitti', **kw).frame_size()
        augs = {c: augment.RainAugment('kitti', lens=lens.LensDrops(H, W, count=c, seed=1), **kw) for c in counts}
        Bmax = max(batches)
        base = np.stack([(synthetic.make_frame(i, H, W)[..., ::-1] * 255).astype(np.uint8) for i in range(8)])
        img8 = torch.from_numpy(np.ascontiguousarray(base.transpose(0, 3, 1, 2))).to(dev)
        img8 = img8.repeat((Bmax + 7) // 8, 1, 1, 1)[:Bmax].contiguous()
        depth = (torch.linspace(80.0, 2.0, H, device=dev)[:, None] * torch.ones((1, W), device=dev)).expand(Bmax, H, W).contiguous()
        for dt in ('uint8', 'float32'):
            img = img8 if dt == 'uint8' else (img8.float() / 255.0)
            for B in batches:
                x, d = img[:B], depth[:B]
                idx = np.arange(B) * 7                           # random access: every image another table
                per = {c: dict(lens=[], kernel=[], rain=[]) for c in counts}
                shown = {}

                def one(c, timed):
                    aug = augs[c]
                    if aug._hip is None:                         # the first call makes the context
                        aug(x, d, a.intensity, idx)
                    aug._hip.profile(True)
                    aug._hip.profile_reset()
                    for _ in range(a.calls):
                        aug(x, d, a.intensity, idx)
                    torch.cuda.synchronize()
                    st = aug._hip.profile_read()
                    aug._hip.profile(False)
                    assert 'k_lens_drops' in st, sorted(st)
                    shown[c] = float(np.mean([len(aug.lens.table(int(f))) for f in idx]))
                    if timed:
                        per[c]['lens'].append(sum(st.get(k, (0, 0.0))[1] for k in LENS) / a.calls)
                        per[c]['kernel'].append(st['k_lens_drops'][1] / a.calls)
                        per[c]['rain'].append(sum(v[1] for k, v in st.items() if k not in LENS) / a.calls)
                for c in counts:                                 # warm-up
                    one(c, False)
                for _ in range(a.rounds):
                    for c in counts:
                        one(c, True)
                for c in counts:
                    res = dict(dtype=dt, B=B, count=c, drops_shown_per_frame=round(shown[c], 1), lens_pass=_stats(per[c]['lens']),
                               k_lens_drops=_stats(per[c]['kernel']), rain_step=_stats(per[c]['rain']))
                    res['lens_over_rain'] = round(res['lens_pass']['median'] / res['rain_step']['median'], 4)
                    out['cases'].append(res)
                    rows.append('| %s | %d | %d | %.1f | %s | %s | %s | %.4f |' % (dt, B, c, shown[c], _cell(res['lens_pass']), _cell(res['k_lens_drops']),
                                                                                 _cell(res['rain_step']), res['lens_over_rain']))
        for aug in augs.values():
            aug.close()
    print(json.dumps(out), flush=True)
    if a.md:
        with open(a.md, 'a') as fh:
            fh.write('\nRainAugment(lens=), KITTI %g mm/hr, %d rounds of %d calls, ms per call: median [min .. max]\n\n' % (a.intensity, a.rounds, a.calls))
            fh.write('| dtype | B | count | drops shown per frame | lens pass (copy + kernel) | k_lens_drops | rain step | lens / rain |\n')
            fh.write('|---|---|---|---|---|---|---|---|\n')
            fh.write('\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
