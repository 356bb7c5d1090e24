#!/usr/bin/env python3
"""CPU model of k_fov_dda's vertex path: which drops should share a wave?

k_fov_dda walks a drop's field-of-view polygon down the rows of the environment map, one lane per drop.  The wave
executes the walk's vertex path -- a hand-over of 24 / 27 vector instructions per side on top of the row's 45 (before the
records became a chain: about 220 of ~300 per row) -- on every row on which ANY of its 64 polygons has a vertex.  This script counts those wave-rows for a frame of the headline workload under several orders of
the drops, so that a sort key can be tried here before the kernel is touched (k_fov_vertices writes the key, k_fov_sort
sorts by it; the key must be a pure function of the drop's record and the camera).

Frame 0 of the headline simulation (synthetic.simulate_particles, 8192 drops, seed 3000), polygons from
oracle/render.compute_fov_plane_points on the 375 x 1909 map; the drops all of whose 20 vertices lie on the map are
grouped 64 at a time.  Measured with this script (fraction of a wave's map rows on which some lane has a vertex; rows
outside the union of the wave's polygons):

    order of the drops                                   vertex rows   rows outside
    table order (the kernel before the sort)                0.888         0.07
    by top row, then bottom row                             0.692         0.17
    by all sorted vertex rows, lexicographic                0.623         0.16
    by distance in 0.25 m buckets, then top row (default)   0.597         0.18

The first line is what the counters showed for the kernel in table order (89 %: profiles/r06_ab_log.md section 3), so
the model counts the right thing.  With ~45 straight-path instructions per wave-row and ~34 more on a vertex row (static
count of the row loop: 24 / 27 per side that takes an edge, 1.33 sides per vertex row; SQ_INSTS_VALU: 1.37 G per launch, of
which the record-making prologue is 0.19 G -- profiles/fov_walk_cost.md) the order takes an eighth off the row loop's
instructions at 0.60: (45 + 34 x 0.597) / (45 + 34 x 0.888) = 0.87.  (With the walker before, ~80 and ~247: a quarter.)  Keys tried and no better than 0.56 .. 0.60: other bucket widths
(0.35 m: 0.593; 0.125 m: 0.668), the polygon's height in place of the distance (height / 8, top row: 0.565; top row / 4,
height: 0.559), the middle row in place of the top row (0.579): the polygon depends on three continuous parameters and a
frame holds 113 waves.

    python scripts/fov_order_model.py [--drops 8192] [--seed 3000] [--height 375] [--width 1242]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
synthetic = importlib.import_module('rain-rendering_amd.synthetic')
from oracle import render as orc  # noqa: E402

WAVE = 64


def polygons(n_drops, seed, H, W, focal_mm=6.0):
    """(vertex rows (n, 20) int, distance (n,) in metres) of the frame's drops whose 20 vertices all lie on the map."""
    He, We = H, synthetic.envmap_width(focal_mm, W)
    fr = synthetic.simulate_particles(1, n_drops, W, H, focal_mm=focal_mm, seed0=seed)[0]
    rows, dist = [], []
    for d in fr['drops']:
        # the loader's world coordinates: z negated (bad_weather.py:223-224)
        wps = np.array([d['wp1'][0], d['wp1'][1], -d['wp1'][2]])
        wpe = np.array([d['wp2'][0], d['wp2'][1], -d['wp2'][2]])
        pts = orc.compute_fov_plane_points(wps, wpe, orc.RADIUS, orc.FOV_DEG, orc.N_FOV, (He, We))
        if len(pts) != orc.N_FOV or not np.all(np.isfinite(pts)):
            continue                                   # no polygon, or a wrapping one: k_fov_spans' drops
        ix, iy = pts[:, 0].astype(int), pts[:, 1].astype(int)
        if ix.min() < 0 or ix.max() >= We or iy.min() < 0 or iy.max() >= He:
            continue
        rows.append(iy)
        dist.append(np.linalg.norm((wps + wpe) / 2))
    return np.array(rows), np.array(dist), He


# ---- sort keys: each returns the order (a permutation of the drops); ties keep the table order ----
def key_table(rows, dist):
    return np.arange(len(rows))


def key_top_bottom(rows, dist):
    return np.lexsort((rows.max(1), rows.min(1)))


def key_vertex_rows(rows, dist):
    s = np.sort(rows, axis=1)
    return np.lexsort(s.T[::-1])


def key_distance_top(rows, dist, bucket_m=0.25):
    return np.lexsort((rows.min(1), np.minimum((dist / bucket_m).astype(int), 62)))


KEYS = (('table order', key_table), ('top row, bottom row', key_top_bottom), ('sorted vertex rows, lexicographic', key_vertex_rows),
        ('distance in 0.25 m buckets, top row', key_distance_top))


def wave_rows(rows, order, He):
    """(fraction of wave-rows with a vertex of some lane, fraction outside the union of the wave's row ranges)."""
    vert = outside = total = 0
    for a in range(0, len(order), WAVE):
        r = rows[order[a:a + WAVE]]
        vert += len(np.unique(r))
        outside += He - (r.max() - r.min() + 1)
        total += He
    return vert / total, outside / total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--drops', type=int, default=8192)
    ap.add_argument('--seed', type=int, default=3000)
    ap.add_argument('--height', type=int, default=375)
    ap.add_argument('--width', type=int, default=1242)
    args = ap.parse_args()
    rows, dist, He = polygons(args.drops, args.seed, args.height, args.width)
    tall = rows.max(1) - rows.min(1) + 1
    print('%d of %d drops with all %d vertices on the map; %.0f rows tall, %.1f distinct vertex rows on average' %
          (len(rows), args.drops, orc.N_FOV, tall.mean(), np.mean([len(np.unique(r)) for r in rows])))
    print('%-40s %12s %13s' % ('order of the drops', 'vertex rows', 'rows outside'))
    for name, key in KEYS:
        v, o = wave_rows(rows, key(rows, dist), He)
        print('%-40s %12.3f %13.3f' % (name, v, o))


if __name__ == '__main__':
    main()
