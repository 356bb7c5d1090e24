"""Cost of the tensor formats of RainAugment: a channels-last uint8 batch and a planar bfloat16 batch through the
library's own ingest and finalize stages, against the route a caller had to take before them -- a conversion to a planar uint8 /
float32 batch in front of the call and one back behind it.  One process, KITTI frames (1242 x 375), --rate mm/hr, batch --batch:

  planar_u8          the call on planar uint8 (the yardstick: what the call costs with no conversion at all)
  cl_u8              the call on channels-last uint8
  cl_u8_converted    x.contiguous() + the call + rainy.contiguous(memory_format=torch.channels_last)
  bf16               the call on planar bfloat16
  bf16_converted     x.float() + the call + rainy.to(torch.bfloat16)

Every variant is warmed up, then the variants alternate for --rounds rounds; a round times each variant between two device events
on the current stream (the call itself ends in a wait for its batch).  Reported: ms per call as median [min .. max] -- the spread of
repeated identical calls -- and the bytes the stages at the two ends of a call move per frame, from the shapes.  The results of the
two routes are compared bit for bit before anything is timed.  Then the two end stages alone for each of the eight formats: us per
frame of the ingest kernel (k_planar_in or k_tensor_in) and of k_finalize_planar from the library profile (HIP events around each launch), median of
--rounds calls.  Needs a GPU: without one the script fails.

Prints one JSON line; --md appends the same figures to a markdown file.  Informational: nothing is gated on the figures.

  python scripts/tensor_formats_cost.py [--batch 32] [--rounds 15] [--rate 25] [--md FILE]
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

H, W = 375, 1242


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def _cell(s):
    return '%.4g [%.4g .. %.4g]' % (s['median'], s['min'], s['max'])


def stage_bytes(el, converted):
    """Bytes per frame read + written by the stages at the two ends of a call for elements of `el` bytes: ingest (the batch in, the
    scratch image out: bytes stay bytes, everything else becomes float32) and finalize's image store; `converted`: plus the two
    torch copies of the conversion route (each reads one format and writes the other) around a planar uint8 / float32 call."""
    px = H * W * 3
    if not converted:
        return px * el + px * (1 if el == 1 else 4) + px * el
    call_el = 1 if el == 1 else 4
    return 2 * (px * el + px * call_el) + stage_bytes(call_el, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--rate', type=int, default=25)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    import torch                                         # (before the library: one HIP runtime per process)
    if not torch.cuda.is_available():
        raise SystemExit('tensor_formats_cost.py measures on a GPU: none found')
    import __graft_entry__ as ge
    ge.build()
    augment = importlib.import_module('rain-rendering_amd.augment')
    synthetic = importlib.import_module('rain-rendering_amd.synthetic')
    dev = torch.device('cuda', 0)
    B = a.batch
    CL = torch.channels_last
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
        aug = augment.RainAugment('kitti', streaks_db=os.path.join(tmp, 'rainstreakdb'), sequence='data_object/training')
        frames = np.stack([(synthetic.make_frame(i, H, W) * 255).astype(np.uint8) for i in range(min(B, 8))])
        x8 = torch.from_numpy(np.ascontiguousarray(frames[np.arange(B) % len(frames)][..., ::-1].transpose(0, 3, 1, 2))).to(dev)
        depth = torch.from_numpy((np.linspace(80.0, 2.0, H)[:, None] * np.ones((1, W))).astype(np.float32)).to(dev).expand(B, H, W).contiguous()
        x8_cl = x8.contiguous(memory_format=CL)
        xbf = (x8.float() / 255.0).to(torch.bfloat16)
        idx = list(range(B))
        variants = {
            'planar_u8': lambda: aug(x8, depth, a.rate, idx)[0],
            'cl_u8': lambda: aug(x8_cl, depth, a.rate, idx)[0],
            'cl_u8_converted': lambda: aug(x8_cl.contiguous(), depth, a.rate, idx)[0].contiguous(memory_format=CL),
            'bf16': lambda: aug(xbf, depth, a.rate, idx)[0],
            'bf16_converted': lambda: aug(xbf.float(), depth, a.rate, idx)[0].to(torch.bfloat16),
        }
        # warm-up of every shape, and the two routes give the same bits
        outs = {}
        for name, fn in variants.items():
            for _ in range(3):
                outs[name] = fn()
        torch.cuda.synchronize()
        same = dict(cl_u8=bool(torch.equal(outs['cl_u8'], outs['cl_u8_converted']) and torch.equal(outs['cl_u8'], outs['planar_u8'])),
                    bf16=bool(torch.equal(outs['bf16'], outs['bf16_converted'])))
        assert outs['cl_u8'].is_contiguous(memory_format=CL) and not outs['cl_u8'].is_contiguous() and all(same.values()), same
        del outs
        ms = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        # the two end stages alone, every format (profiled calls: not part of the timings above)
        hip = aug._hip
        kern = {}
        xs = {'uint8': x8, 'float32': x8.float() / 255.0, 'float16': (x8.float() / 255.0).half(), 'bfloat16': xbf}
        for dt, xp in xs.items():
            for lay, x in (('planar', xp), ('interleaved', xp.contiguous(memory_format=CL))):
                aug(x, depth, a.rate, idx)
                ingest = 'k_planar_in' if lay == 'planar' and dt in ('uint8', 'float32') else 'k_tensor_in'
                per = {ingest: [], 'k_finalize_planar': []}
                for _ in range(a.rounds):
                    hip.profile(True)
                    hip.profile_reset()
                    aug(x, depth, a.rate, idx)
                    stt = hip.profile_read()
                    hip.profile(False)
                    for k in per:
                        per[k].append(1e3 * stt[k][1] / stt[k][0] / B)
                kern['%s %s' % (dt, lay)] = dict(ingest_us_per_frame=_stats(per[ingest]), finalize_us_per_frame=_stats(per['k_finalize_planar']))
        aug.close()
    st = {name: _stats(v) for name, v in ms.items()}
    el = dict(planar_u8=(1, False), cl_u8=(1, False), cl_u8_converted=(1, True), bf16=(2, False), bf16_converted=(2, True))
    out = dict(what='RainAugment tensor formats: %dx%d, %d mm/hr, batch %d, %d alternating rounds' % (W, H, a.rate, B, a.rounds),
               device=torch.cuda.get_device_name(0), same_bits=same, ms_per_call=st,
               frames_per_s={k: round(B / (v['median'] * 1e-3), 1) for k, v in st.items()},
               spread_of_identical_calls={k: round((v['max'] - v['min']) / v['median'], 4) for k, v in st.items()},
               end_stage_bytes_per_frame={k: stage_bytes(*v) for k, v in el.items()}, end_stages=kern,
               direct_over_converted=dict(cl_u8=round(st['cl_u8']['median'] / st['cl_u8_converted']['median'], 4),
                                          bf16=round(st['bf16']['median'] / st['bf16_converted']['median'], 4)))
    print(json.dumps(out), flush=True)
    if a.md:
        with open(a.md, 'a') as fh:
            fh.write('\n%s (%s); ms per call: median [min .. max]\n\n' % (out['what'], out['device']))
            fh.write('| variant | ms per call | frames/s | (max - min) / median | bytes moved per frame by the end stages |\n|---|---|---|---|---|\n')
            for k in variants:
                fh.write('| %s | %s | %.1f | %.4f | %d |\n' % (k, _cell(st[k]), out['frames_per_s'][k], out['spread_of_identical_calls'][k],
                                                              out['end_stage_bytes_per_frame'][k]))
            fh.write('\nthe two end stages alone (library profile), us per frame: median [min .. max]\n\n')
            fh.write('| format | ingest (k_planar_in / k_tensor_in) | k_finalize_planar |\n|---|---|---|\n')
            for k, v in kern.items():
                fh.write('| %s | %s | %s |\n' % (k, _cell(v['ingest_us_per_frame']), _cell(v['finalize_us_per_frame'])))
            fh.write('\nmedian of the direct call over the conversion route: channels-last uint8 %.4f, bfloat16 %.4f; the two routes gave '
                     'equal bits: %s\n' % (out['direct_over_converted']['cl_u8'], out['direct_over_converted']['bf16'], same))


if __name__ == '__main__':
    main()
