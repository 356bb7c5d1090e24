"""Writes profiles/colour_route_accuracy.md: per case of the colour catalogue (tests/colour_cases.py) the largest rounding bound,
the largest error / bound of the float32 restatement on the CPU and -- from the output of the GPU tier
(`pytest tests/test_gpu_colour_cases.py -m gpu -s`, its `colour-accuracy` lines) -- of the device, and the exception drops
against their cap.

    python scripts/colour_route_accuracy.py [gpu_tier_output.log]"""
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import colour_cases as col  # noqa: E402
import test_colour_cases_host as tch  # noqa: E402


def device_figures(path):
    """case -> dict(ratio, exceptions, cap, f64): the worst over the case's calls."""
    out = {}
    for line in open(path):
        m = re.search(r'colour-accuracy (\S+) (.*)', line)
        if not m:
            continue
        d = out.setdefault('big' if m.group(1) == 'batch' else m.group(1), dict(ratio=0.0, exceptions=0, cap=0, f64=0.0, calls=0))
        d['calls'] += 1
        r = re.search(r'error / bound=([\d.]+).*exceptions=(\d+) cap=(\d+)', m.group(2))
        if r:
            d['ratio'] = max(d['ratio'], float(r.group(1)))
            if int(r.group(2)) >= d['exceptions']:
                d['exceptions'], d['cap'] = int(r.group(2)), int(r.group(3))
        r = re.search(r'max\|K\|=([\d.e+-]+)', m.group(2))
        if r:
            d['f64'] = max(d['f64'], float(r.group(1)))
    return out


def main():
    dev = device_figures(sys.argv[1]) if len(sys.argv) > 1 else {}
    with tempfile.TemporaryDirectory() as tmp:
        def tmp_of(n):
            p = os.path.join(tmp, n)
            os.makedirs(p)
            return p
        cat = col.build(col.Base(tmp_of))
        rows, shares = [], {}
        for name, c in cat.items():
            fast = col.predict(c.He, c.We, (max(c.n, 1),))['fast']
            worst_b, worst_r = np.zeros(3), 0.0
            for rule in ((1, 0) if 'placement' in c.aims else (1,)):
                r = c.ref(rule)
                comp = r['composited']
                worst_b = np.maximum(worst_b, (r['bound'][comp] / np.abs(r['xyY'][comp])).max(axis=0))
                if fast:
                    xl, xr = c.spans(rule)
                    S, sw, sy = col.float_sums(c.map, xl, xr)
                    worst_r = max(worst_r, float((np.abs(col.xyY_of_sums(S, sw, sy) - r['xyY'])[comp] / r['bound'][comp]).max()))
                    for label, fn, aim in tch.MISTAKES:
                        if aim is not None and aim not in c.aims:
                            continue
                        sizes = ((2500, 834), (col.BIG_N, 4097), (1025, 513), (2049, 1025)) if aim in ('chunks', 'order') else ((c.n, c.n),)
                        for n, per in sizes:
                            S2, touched = fn(c, rule, n, per)
                            touched = touched & comp[:n]
                            left = tch._left(dict(xyY=r['xyY'][:n], bound=r['bound'][:n]), col.xyY_of_sums(S2, c.map.sumW, c.map.sumY))
                            share = (left & touched).sum() / touched.sum()
                            if share < shares.get(label, (2.0, ''))[0]:
                                shares[label] = (float(share), name)
            d = dev.get(name, {})
            rows.append((name, c.He, c.We, c.cone, 'float32' if c.env32 else 'float64', c.n, worst_b, worst_r if fast else None, d))
    out = ['# The colour branch against a float64 reference: bounds and observed errors', '',
           'Written by `scripts/colour_route_accuracy.py` from the catalogue of `tests/colour_cases.py`.  The bound is the one its',
           'docstring derives from the summation order of `k_fov_sums32` (u = 2^-24; nothing fitted to a device result); it is',
           'stated relative to the drop\'s own (x, y, Yg), the largest over the case\'s composited drops.  `CPU` is the float32',
           'restatement of the row scan\'s structure (tests/test_colour_cases_host.py), `device` the MI355X through the C ABI',
           '(tests/test_gpu_colour_cases.py, the worst of the case\'s calls: drops per thread, order, walk, fill rule, batch).',
           'An exception is a drop outside the bound that a polygon one vertex and one texel away explains (the device\'s float',
           'vertices truncate to another texel); the cap is 1 % of the composited drops, 3 below 300.  `float64` is the largest',
           '|K - reference| / max|K| of the case\'s float64 calls (bar: 1e-9).', '',
           '| case | map (He x We) | cone | map type | drops | bound x | bound y | bound Yg | CPU error / bound | device error / bound | exceptions / cap | float64 |',
           '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for name, He, We, cone, typ, n, b, r, d in rows:
        out.append('| %s | %d x %d | %d | %s | %d | %.2e | %.2e | %.2e | %s | %s | %s | %s |' % (
            name, He, We, cone, typ, n, b[0], b[1], b[2], '%.3f' % r if r is not None else 'general path',
            '%.3f' % d['ratio'] if d.get('cap') else '-', '%d / %d' % (d['exceptions'], d['cap']) if d.get('cap') else '-',
            '%.1e' % d['f64'] if d.get('f64') else '-'))
    worst = max(rows, key=lambda t: max(t[6][:2]))
    out += ['', 'The largest bound of the float route is that of `%s` (%d x %d, the %d-degree cone): %.1e relative on x and y.  A span\'s'
            % (worst[0], worst[1], worst[2], worst[3], max(worst[6][:2])),
            'error grows with (row total / span sum), and the narrow cone\'s spans are a few per cent of a row.  The product\'s',
            '165-degree cone stays at or under %.1e on every map of the fast path.' % max(max(t[6][:2]) for t in rows if t[3] == 165 and t[7] is not None), '',
            '## How sharp the bound is', '',
            'Each mistake applied to the float64 reference; the smallest share, over the cases that aim at it, of the touched drops',
            'that leave the bound (the CPU tier asserts >= 0.9):', '', '| mistake | smallest share | in case |', '|---|---|---|']
    for label, fn, aim in tch.MISTAKES:
        out.append('| %s | %.3f | %s |' % (label, shares[label][0], shares[label][1]))
    with open(os.path.join(ROOT, 'profiles', 'colour_route_accuracy.md'), 'w') as fh:
        fh.write('\n'.join(out) + '\n')
    print('\n'.join(out[-12:]))


if __name__ == '__main__':
    main()
