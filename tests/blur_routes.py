"""Which defocus-blur route every drop of a frame takes, decided on the host the way the kernels decide it, and a catalogue of
hand-built drops that reaches every route and both sides of each threshold.

Routes (rainhip.hip make_list_rec / k_lists, rr_device.h blur_is_small / blur_layout):
  no_blur       r1 == 0 and shift == 0: the drop's tile is used as it is
  pad_only      r1 == 0 < shift = int(10 c), c in [0.1, 0.125): the reference pads, nothing is filtered
  small         k_blur_small: one wave per drop
  fused_single  k_blur_fused_dma: one sub-tile covers the effective tile (filtered in place)
  fused_bands   k_blur_fused_dma: full-width bands of rows
  fused_2d      k_blur_fused_dma: 2-D sub-tiles (wide tile, large radius)
  slow_radius   k_blur_big_weights + k_blur<0>, k_blur<1>: r1 > BR_MAX
  slow_halo     the same: r1 <= BR_MAX, but no sub-tile fits the LDS capacities
  too_big       RR_DROP_TOO_BIG: 10 c >= RR_MAX_SHIFT + 1, skipped
  skipped       any other status, or nothing of the drop is rendered (no FOV polygon, footprint outside the frame)
and, across routes, the flags
  row_r0        r2 == 0 < r1 (c in [0.125, 0.25)): the row pass has radius 0
  split         a fused drop of more than BLUR_ITEMS_PER_DROP sub-tiles: several sub-tiles per work item
  zero_item     ... and one of its items has no sub-tile at all (imax(imin(per, ns - st0), 0), k_lists)
  partial_band  the last band (or row of 2-D sub-tiles) is shorter than the others
  beyond_cap    a slow drop past the frame's first SLOW_CAP slow drops (k_blur builds its own weight tables)

The LDS capacities come from the host build of rr_device.h (emu_blur_capacities), SLOW_CAP and BLUR_ITEMS_PER_DROP from
rainhip.hip, so a build with other values is classified the way it runs."""
import ctypes
import os
import re

import numpy as np

import helpers as h

RR_DROP_OK, RR_DROP_TOO_BIG = 0, 4
KIND_BIG = 0
MAX_SHIFT = 1024                        # include/rainhip.h RR_MAX_SHIFT

ROUTES = ('no_blur', 'pad_only', 'small', 'fused_single', 'fused_bands', 'fused_2d', 'slow_radius', 'slow_halo', 'too_big', 'skipped')
FLAGS = ('row_r0', 'split', 'zero_item', 'partial_band', 'beyond_cap')
FUSED = ('fused_single', 'fused_bands', 'fused_2d')
SLOW = ('slow_radius', 'slow_halo')


def _hip_constant(name):
    src = open(os.path.join(h.ROOT, 'rain-rendering_amd', 'csrc', 'rainhip.hip')).read()
    m = re.search(r'constexpr int %s = (\d+);' % name, src)
    assert m, name
    return int(m.group(1))


SLOW_CAP = _hip_constant('SLOW_CAP')
ITEMS_PER_DROP = _hip_constant('BLUR_ITEMS_PER_DROP')


def capacities():
    emu = h.hostemu()
    cap = np.zeros(2, np.int32)
    emu.emu_blur_capacities(h._p(cap))
    return int(cap[0]), int(cap[1])


def blur_layout(ew, eh, r1, r2, tw, th, caps=None):
    """(small, fused, wo, ho) of one effective tile: rr_device.h blur_is_small / blur_layout through the host build."""
    emu = h.hostemu()
    bx, by = caps or capacities()
    out = np.zeros(4, np.int32)
    emu.emu_blur_layout.argtypes = [ctypes.c_int] * 8 + [ctypes.c_void_p]
    assert emu.emu_blur_layout(int(ew), int(eh), int(r1), int(r2), int(tw), int(th), bx, by, h._p(out)) == 0
    return tuple(int(v) for v in out)


def item_split(ns):
    """The work items k_lists makes of a fused drop of ns sub-tiles: (first sub-tile, number of sub-tiles) each."""
    ni = min(ns, ITEMS_PER_DROP)
    per = (ns + ni - 1) // ni
    return [(k * per, max(min(per, ns - k * per), 0)) for k in range(ni)]


def classify(plans, sizes, caps=None):
    """One record per drop: the plan fields the route depends on, the route, the flags, the fused layout and its items,
    the slow drop's rank in the frame's slow list, and the footprint (x0, y0, x1, y1) the drop can touch."""
    caps = caps or capacities()
    recs, slow_rank = [], 0
    for i, p in enumerate(plans):
        r = dict(i=i, status=int(p['status']), kind=int(p['kind']), tw=int(p['tw']), th=int(p['th']), shift=int(p['shift']),
                 r1=int(p['r1']), r2=int(p['r2']), ew=int(p['ew']), eh=int(p['eh']), live=bool(p['status'] == RR_DROP_OK and sizes[i] > 0),
                 ns=0, wo=0, ho=0, items=[], slow_rank=None, flags=set())
        # the effective tile (where the blurred alpha can be non-zero) on the frame: it starts (shift - r2, shift - r1) into the
        # padded tile, whose visible part starts (crop_x, crop_y) into it at (vis_x0, vis_y0)
        vx0, vy0, vx1, vy1 = int(p['vis_x0']), int(p['vis_y0']), int(p['vis_x0'] + p['vis_w']), int(p['vis_y0'] + p['vis_h'])
        ex0 = vx0 - int(p['crop_x']) + r['shift'] - r['r2']
        ey0 = vy0 - int(p['crop_y']) + r['shift'] - r['r1']
        r['box'] = (max(vx0, ex0), max(vy0, ey0), min(vx1, ex0 + r['ew']), min(vy1, ey0 + r['eh']))
        if r['status'] == RR_DROP_TOO_BIG:
            r['route'] = 'too_big'
        elif not r['live']:
            r['route'] = 'skipped'
        elif r['r1'] == 0:
            r['route'] = 'pad_only' if r['shift'] > 0 else 'no_blur'
        else:
            small, fused, wo, ho = blur_layout(r['ew'], r['eh'], r['r1'], r['r2'], r['tw'], r['th'], caps)
            if r['r2'] == 0:
                r['flags'].add('row_r0')
            if small:
                r['route'] = 'small'
            elif fused:
                r.update(wo=wo, ho=ho, ns=-(-r['ew'] // wo) * -(-r['eh'] // ho))
                r['route'] = 'fused_single' if r['ns'] == 1 else 'fused_bands' if wo >= r['ew'] else 'fused_2d'
                r['items'] = item_split(r['ns'])
                if r['ns'] > ITEMS_PER_DROP:
                    r['flags'].add('split')
                if any(n == 0 for _, n in r['items']):
                    r['flags'].add('zero_item')
                if r['ns'] > 1 and r['eh'] % ho:
                    r['flags'].add('partial_band')
            else:
                r['route'] = 'slow_radius' if r['r1'] > 48 else 'slow_halo'
                r['slow_rank'] = slow_rank
                if slow_rank >= SLOW_CAP:
                    r['flags'].add('beyond_cap')
                slow_rank += 1
        recs.append(r)
    return recs


def classify_drops(scene, drops, polygon_gate=False):
    """classify() of a frame's drops.  The library's default schedule (RR_OPT_COLOUR_STREAM 1) plans the tiles before the FOV
    polygons are known: a drop without a polygon still gets its tile and its place in the work lists (it is not blended).
    polygon_gate=True classifies the way the one-stream schedule runs (such a drop renders nothing)."""
    plans, sizes = h.emu_plan(scene, drops)
    if not polygon_gate:
        sizes = ((plans['status'] == RR_DROP_OK) & (plans['vis_w'] > 0) & (plans['vis_h'] > 0)).astype(np.int64)
    return classify(plans, sizes)


def expected_counts(recs):
    """rr_batch_counts [2] .. [6] of a frame rendered with RR_OPT_DEDUP 0 (every drop renders its own raw tile): fused work
    items, slow drops, small drops, Big tiles and their pixels."""
    live = [r for r in recs if r['live']]
    return [sum(len(r['items']) for r in live if r['route'] in FUSED), sum(r['route'] in SLOW for r in live),
            sum(r['route'] == 'small' for r in live), sum(r['kind'] == KIND_BIG for r in live),
            sum(r['tw'] * r['th'] for r in live if r['kind'] == KIND_BIG)]


def census(recs):
    """{route or flag: number of drops}."""
    out = {k: 0 for k in ROUTES + FLAGS}
    for r in recs:
        out[r['route']] += 1
        for f in r['flags']:
            out[f] += 1
    return out


def routes_touching(recs, diff):
    """{route: number of its drops whose footprint holds a pixel where `diff` (H x W bool) is set}: which part of the blur a
    failing comparison points at."""
    ys, xs = np.nonzero(diff)
    out = {}
    for r in recs:
        x0, y0, x1, y1 = r['box']
        if r['live'] and len(xs) and ((xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)).any():
            key = r['route'] + ''.join('+' + f for f in sorted(r['flags']))
            out[key] = out.get(key, 0) + 1
    return out


def check(out, ref, recs, tag):
    """The bars of test_gpu_parity._check -- statuses equal, mask and mask_i32 bit-exact, image_u8 within 1 LSB, rainy_bg within
    1e-9 -- and on failure the routes whose drops touch the differing pixels."""
    assert np.array_equal(out['status'], ref['status']), '%s status: %s' % (tag, [(recs[i]['route'], int(out['status'][i]), int(ref['status'][i]))
                                                                                for i in np.nonzero(out['status'] != ref['status'])[0][:8]])
    where = {}
    for key, diff in (('mask', out['mask'] != ref['mask']), ('mask_i32', out['mask_i32'] != ref['mask_i32']),
                      ('image_u8', (np.abs(out['image_u8'].astype(int) - ref['image_u8'].astype(int)) > 1).any(axis=2)),
                      ('rainy_bg', (np.abs(out['rainy_bg'] - ref['rainy_bg']) >= 1e-9).any(axis=2))):
        if diff.any():
            where[key] = '%d px on the drops of %s' % (diff.sum(), routes_touching(recs, diff))
    assert not where, '%s differs: %s' % (tag, where)


# ---------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------
def coc_for_radius(r1):
    """A circle of confusion whose r1 = int(4 c + 0.5) is r1, away from every rounding boundary of r1, r2 and shift."""
    return r1 / 4.0 + 0.05


# (name, expected route, expected flags, big?, x0, y0, tw, th, c); Big drops are 5 px wide (tw = dx + 5), the others are
# vertical 2.5 px streaks (tw = 4) unless tw says otherwise (an oblique streak dx = tw wide)
CATALOGUE = [
    ('in_focus', 'no_blur', (), False, 20, 30, 4, 40, 0.0),
    ('pad_only', 'pad_only', (), False, 40, 30, 4, 40, 0.11),
    ('row_radius_0', 'small', ('row_r0',), False, 60, 30, 4, 40, 0.2),
    ('small_oblique', 'small', (), False, 80, 30, 9, 20, 1.0),
    ('small_bs_x_512', 'small', (), True, 110, 30, 16, 16, coc_for_radius(4)),      # tw (php + 2 r1) = 16 * 32 = 512 = BS_X
    ('fused_bs_x_576', 'fused_single', (), True, 140, 30, 16, 17, coc_for_radius(4)),  # the next row: 16 * 36 (the product is even)
    ('fused_single', 'fused_single', (), True, 170, 30, 20, 30, coc_for_radius(8)),
    ('bands_8', 'fused_bands', ('partial_band',), True, 200, 60, 19, 352, coc_for_radius(8)),
    ('bands_9', 'fused_bands', ('split', 'zero_item', 'partial_band'), True, 230, 50, 22, 373, coc_for_radius(8)),
    ('bands_17', 'fused_bands', ('split', 'zero_item', 'partial_band'), True, 270, 50, 58, 373, coc_for_radius(8)),
    ('subtiles_2d', 'fused_2d', ('split', 'zero_item', 'partial_band'), True, 340, 40, 60, 4, coc_for_radius(20)),
    ('r1_31', 'fused_2d', ('split', 'zero_item'), True, 420, 100, 4, 10, coc_for_radius(31)),
    ('r1_32', 'fused_2d', ('split', 'partial_band'), True, 470, 100, 4, 10, coc_for_radius(32)),
    ('r1_48', 'slow_halo', (), True, 520, 100, 10, 30, coc_for_radius(48)),
    ('r1_49', 'slow_radius', (), True, 560, 200, 10, 30, coc_for_radius(49)),
    ('slow_wide', 'slow_radius', (), True, 380, 300, 100, 40, coc_for_radius(60)),    # tw > BIG_GROUPS: a unit takes two columns
    ('halo_wide', 'slow_halo', (), True, 450, 400, 80, 20, coc_for_radius(40)),
    ('too_big_1025', 'too_big', (), True, 300, 250, 8, 10, (MAX_SHIFT + 1) / 10.0 + 0.05),
    # frame borders: the blurred tile is cropped on every side
    ('left_small', 'small', (), False, 0, 200, 4, 24, 1.0),
    ('left_fused', 'fused_single', (), True, -2, 260, 12, 30, coc_for_radius(8)),
    ('top_fused_2d', 'fused_2d', ('split', 'zero_item', 'partial_band'), True, 100, 0, 40, 6, coc_for_radius(24)),
    ('right_bands', 'fused_bands', (), True, 630, 120, 12, 300, coc_for_radius(10)),
    ('bottom_slow', 'slow_radius', (), True, 150, 450, 30, 30, coc_for_radius(52)),
    ('bottom_right_halo', 'slow_halo', (), True, 600, 440, 40, 40, coc_for_radius(44)),
    ('top_left_small', 'small', (), False, 2, 0, 4, 12, 0.8),
    ('bottom_small', 'small', ('row_r0',), False, 300, 470, 4, 10, 0.2),
]
CAT_H, CAT_W = 480, 640
# the boundary of RR_DROP_TOO_BIG: int(10 c) = 1024 is rendered (r1 ~ 410, a padded tile of ~2100 x 2100) -- a frame of its own
BOUNDARY = [('too_big_1024', 'slow_radius', (), True, 60, 20, 8, 240, MAX_SHIFT / 10.0 + 0.05),
            ('too_big_1025', 'too_big', (), True, 100, 20, 8, 10, (MAX_SHIFT + 1) / 10.0 + 0.05)]


def catalogue_particles(entries, H, W, cam=h.KITTI):
    out = []
    for k, (name, route, flags, big, x0, y0, tw, th, c) in enumerate(entries):
        depth = h.depth_for_coc(c, cam) if c > 0 else 6.0
        if big:
            out.append(h.streak(k, x0, y0, x0 + tw - 5, y0 + th, 5.0, 5.0, depth, H, W, cam))
        elif tw > 4:
            out.append(h.streak(k, x0, y0, x0 + tw, y0 + th, 2.5, 2.5, depth, H, W, cam))
        else:
            out.append(h.streak(k, x0, y0, x0, y0 + th, 2.5, 2.5, depth, H, W, cam))
    return out


def slow_cap_particles(n, H, W, seed=5, cam=h.KITTI):
    """n small Big drops on the slow routes at radii 40 .. 56 in random order: with n > SLOW_CAP the drops past the cap
    have other radii than the ones SLOW_CAP places before them."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        r1 = int(rng.randint(40, 57))
        x0, y0 = int(rng.randint(-10, W)), int(rng.randint(-10, H - 4))
        depth = h.depth_for_coc(coc_for_radius(r1), cam)
        out.append(h.streak(k, x0, y0, x0 + int(rng.randint(0, 4)), y0 + int(rng.randint(2, 8)), 5.0, 5.0, depth, H, W, cam))
    return out
