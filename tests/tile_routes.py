"""Which kernel renders every drop's raw alpha tile, decided on the host the way make_list_rec decides it (rr_device.h
tile_class through the host build), and a catalogue of hand-built in-focus drops that reaches every route and both sides of
each threshold.

Routes (rr_device.h tile_class; RR_OPT_TILE_ROWS 0 / 1 / 2 = no k_tile_rows / rotate tiles only / Big tiles too):
  rows        k_tile_rows, row walks, a wave per tile: tile_is_rows
  rot_int     k_tile, integer resize ratios (RS_AREA_FAST): tile_is_fast
  rot         k_tile, any other area resize: tile_is_fast
  gen_area    k_tile_generic, an area resize no other kernel takes
  gen_linear  k_tile_generic, RS_LINEAR: the streak is longer (or wider) than the rotated texture
  big_lds     k_tile_rows' big_tile, a lane per pixel: tile_is_big_lds
  big         k_tile_big: every other Big drop
  skipped     a status, or nothing of the drop is rendered (its footprint lies outside the frame)
and, across routes, the flags
  th_64 th_65 tw_64 tw_65   a rotate tile of exactly that height / width (tile_is_rows: th <= 64; TW_MAX = 64)
  sx_below_2 sx_at_2        a rotate tile with scale_x in [1, 2) / [2, 2.1) (the row walk needs scale_x >= 2)
  chunked                   a rows tile whose rows are cut into several segments of cells (rows_pass_shape: wide tw)
  many_passes               a rows tile of at least 8 passes
  carry                     a rows tile with a destination row whose canvas rows lie in two passes
  flip                      a rotate tile that is mirrored (the canvas rows run backwards)
  big_blocks                a Big tile wider than its block, tw > bw0 (the homography restarts at every block)
  big_px_le_8192 big_px_gt_8192   a Big tile of (BIG_ROWS_MAX_PX - 512, BIG_ROWS_MAX_PX] / (.., + 512] pixels
  big_border                a Big tile with 4 x 4 windows across each of the texture's four sides
  big_one_wave              a Big tile of at most 64 pixels
  tw_1 th_1                 a Big tile one pixel wide / high (cropped by the frame; a streak one row long)

The limits come from the host build of rr_device.h (emu_tile_limits), so a build with other values is classified the way it
runs -- and the catalogue's census (tests/test_tile_routes_host.py) then names the entries that moved."""

import numpy as np

import blur_routes as br
import helpers as h

RR_DROP_OK = 0
KIND_BIG, KIND_ROT = 0, 1
RS_AREA, RS_AREA_FAST, RS_LINEAR = 0, 1, 2
LC_NAMES = {0: 'skipped', 1: 'big_lds', 2: 'big', 3: 'rows', 4: 'rot_int', 5: 'rot', 6: 'gen'}     # rr_device.h LC_*

ROUTES = ('rows', 'rot', 'rot_int', 'gen_area', 'gen_linear', 'big_lds', 'big', 'skipped')
FLAGS = ('th_64', 'th_65', 'tw_64', 'tw_65', 'sx_below_2', 'sx_at_2', 'chunked', 'many_passes', 'carry', 'flip', 'big_blocks',
         'big_px_le_8192', 'big_px_gt_8192', 'big_border', 'big_one_wave', 'tw_1', 'th_1')
K_TILE = ('rot', 'rot_int')
BIG = ('big_lds', 'big')


def limits():
    out = np.zeros(8, np.int32)
    h.hostemu().emu_tile_limits(h._p(out))
    return dict(zip('TEX_LDS NW_MAX TW_MAX BUF_MAX RW_NW RW_BUF RW_PAIR_BYTES BIG_ROWS_MAX_PX'.split(), (int(v) for v in out)))


def db_arrays(scene):
    """(texels, heights, widths, offsets) of the scene's database as the library packs it."""
    return h.hb.pack_streak_db(scene.db.streaks_light)


def tile_classes(plans, hs, ws, tile_rows):
    """rr_device.h tile_class of every plan under RR_OPT_TILE_ROWS `tile_rows`, as route names."""
    emu = h.hostemu()
    out = np.zeros(max(len(plans), 1), np.int32)
    emu.emu_tile_class(h._p(plans), len(plans), h._p(hs), h._p(ws), int(tile_rows >= 1), int(tile_rows >= 2), h._p(out))
    names = []
    for p, c in zip(plans, out):
        n = LC_NAMES[int(c)]
        names.append(('gen_linear' if p['rs_mode'] == RS_LINEAR else 'gen_area') if n == 'gen' else n)
    return names


def classify(plans, live, hs, ws, tile_rows=2):
    """One record per drop: the route (under `tile_rows`, and under every mode in rec['routes']), the plan fields the route
    depends on, the footprint (x0, y0, x1, y1) the in-focus drop can touch, and the flags."""
    emu = h.hostemu()
    lim = limits()
    by_mode = {m: tile_classes(plans, hs, ws, m) for m in (0, 1, 2)}
    recs = []
    for i, p in enumerate(plans):
        ok = bool(live[i])
        routes = {m: by_mode[m][i] if ok else 'skipped' for m in (0, 1, 2)}
        r = dict(i=i, status=int(p['status']), kind=int(p['kind']), live=ok, routes=routes, route=routes[tile_rows], tex=int(p['tex']),
                 tex_h=int(hs[p['tex']]), tex_w=int(ws[p['tex']]), tw=int(p['tw']), th=int(p['th']), nW=int(p['nW']), nH=int(p['nH']),
                 scale_x=float(p['scale_x']), scale_y=float(p['scale_y']), flip=int(p['flip']), bw0=int(p['bw0']), rs_mode=int(p['rs_mode']),
                 box=(int(p['vis_x0']), int(p['vis_y0']), int(p['vis_x0'] + p['vis_w']), int(p['vis_y0'] + p['vis_h'])), flags=set())
        recs.append(r)
        if not ok:
            continue
        fl = np.zeros(5, np.int32)
        emu.emu_tile_flags(h._p(plans[i:i + 1]), h._p(hs), h._p(ws), h._p(fl))
        f = r['flags']
        if r['kind'] == KIND_ROT:
            for k in ('th', 'tw'):
                for v in (64, 65):
                    if r[k] == v:
                        f.add('%s_%d' % (k, v))
            if 1.0 <= r['scale_x'] < 2.0:
                f.add('sx_below_2')
            if 2.0 <= r['scale_x'] < 2.1:
                f.add('sx_at_2')
            if r['flip']:
                f.add('flip')
            if r['route'] == 'rows':
                R, NS, passes, carry = (int(v) for v in fl[:4])
                r.update(R=R, NS=NS, passes=passes)
                if NS > 1:
                    f.add('chunked')
                if r['nH'] / R >= 8:
                    f.add('many_passes')
                if carry:
                    f.add('carry')
        elif r['kind'] == KIND_BIG:
            px = r['tw'] * r['th']
            if r['tw'] > r['bw0']:
                f.add('big_blocks')
            if lim['BIG_ROWS_MAX_PX'] - 512 < px <= lim['BIG_ROWS_MAX_PX']:
                f.add('big_px_le_8192')
            if lim['BIG_ROWS_MAX_PX'] < px <= lim['BIG_ROWS_MAX_PX'] + 512:
                f.add('big_px_gt_8192')
            if int(fl[4]) == 15:
                f.add('big_border')
            if px <= 64:
                f.add('big_one_wave')
            if r['tw'] == 1:
                f.add('tw_1')
            if r['th'] == 1:
                f.add('th_1')
    return recs


def classify_drops(scene, drops, tile_rows=2):
    """classify() of a frame's drops.  As in blur_routes.classify_drops, a drop is live when it has a plan and a footprint on
    the frame: the library's default schedule plans the tiles before the FOV polygons are known."""
    plans, _ = h.emu_plan(scene, drops)
    live = (plans['status'] == RR_DROP_OK) & (plans['vis_w'] > 0) & (plans['vis_h'] > 0)
    _, hs, ws, _ = db_arrays(scene)
    return classify(plans, live, hs, ws, tile_rows)


def expected_counts(recs, tile_rows):
    """rr_batch_counts [0], [1], [5], [6] of a frame rendered with RR_OPT_DEDUP 0 (every drop renders its own raw tile) under
    RR_OPT_TILE_ROWS `tile_rows`: tiles of k_tile_rows + k_tile, of the generic kernel, Big tiles and their pixels."""
    live = [(r, r['routes'][tile_rows]) for r in recs if r['live']]
    return [sum(t in ('rows',) + K_TILE for _, t in live), sum(t in ('gen_area', 'gen_linear') for _, t in live),
            sum(t in BIG for _, t in live), sum(r['tw'] * r['th'] for r, t in live if t in BIG)]


def counts_of(batch_counts):
    """The entries of rr_batch_counts that expected_counts predicts."""
    return [batch_counts[k] for k in (0, 1, 5, 6)]


def census(recs):
    """{route or flag: number of drops}."""
    out = {k: 0 for k in ROUTES + FLAGS}
    for r in recs:
        out[r['route']] += 1
        for f in r['flags']:
            out[f] += 1
    return out


routes_touching = br.routes_touching          # (a record's 'live', 'box', 'route' and 'flags' are all it reads)
check = br.check


# ---------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------
# Frames of the KITTI camera, every drop in focus (depth 6.0: no blur, the mask under a drop is its raw tile), no two
# footprints overlapping.  An entry is (name, expected route under RR_OPT_TILE_ROWS 2, expected flags, x0, y0, dx, dy, image
# width): a streak from (x0, y0) to (x0 + dx, y0 + dy); an image width >= 4 makes a Big drop (tw = |dx| + 5, th = |dy|), a
# smaller one a rotated texture resized to tw = max(|dx|, int(width) + 2) by th = max(|dy|, 2), mirrored ('flip') when it ends
# right of the frame's middle.  The default database's textures are 32 wide and 320, 229, 160, 114 or 80 high; which one a
# drop gets follows from its width / length (DBManager.texture_bucket).  The comments give tw x th, the texture's height and
# scale_x, scale_y = nW / tw, nH / th of the rotated texture.  Neighbouring entries are the two sides of a threshold.
CAT_H, CAT_W = 480, 640
CATALOGUE = {
    # rotate tiles of at most 66 x 66: tile_is_rows' th <= 64 and tw <= 64, TW_MAX, pass shapes, every frame border
    'small': [
        ('rows_thin_8', 'rows', ('carry',), 8, 10, 0, 8, 1.5),   # 3x8 tex 229 sx 10.667 sy 28.625
        ('rows_vertical_20', 'rows', (), 28, 10, 0, 20, 1.5),   # 3x20 tex 320 sx 10.667 sy 16.000
        ('rows_one_pass_wide_8', 'rows', ('carry',), 48, 10, 0, 8, 3.5),   # 5x8 tex 80 sx 6.400 sy 10.000
        ('rot_int_8x8', 'rot_int', (), 68, 10, 0, 40, 2.5),   # 4x40 tex 320 sx 8.000 sy 8.000
        ('rot_int_th_64', 'rot_int', ('th_64',), 88, 10, 0, 64, 2.5),   # 4x64 tex 320 sx 8.000 sy 5.000
        ('rows_th_64', 'rows', ('carry', 'th_64'), 108, 10, 0, 64, 1.5),   # 3x64 tex 320 sx 10.667 sy 5.000
        ('rot_th_65', 'rot', ('th_65',), 128, 10, 0, 65, 1.5),   # 3x65 tex 320 sx 10.667 sy 4.923
        ('rot_th_66', 'rot', (), 148, 10, 0, 66, 1.5),   # 3x66 tex 320 sx 10.667 sy 4.848
        ('rows_th_64_oblique', 'rows', ('carry', 'chunked', 'many_passes', 'th_64'), 168, 10, 12, 64, 1.5),   # 12x64 tex 320 sx 7.500 sy 5.000
        ('rot_th_65_oblique', 'rot', ('th_65',), 192, 10, 12, 65, 1.5),   # 12x65 tex 320 sx 7.417 sy 4.923
        ('rows_leaning_left', 'rows', ('carry', 'chunked', 'many_passes'), 246, 10, -30, 40, 2.5),   # 30x40 tex 320 sx 7.233 sy 6.875
        ('rows_tw_64', 'rows', ('carry', 'chunked', 'many_passes', 'tw_64'), 8, 82, 64, 8, 1.5),   # 64x8 tex 320 sx 5.016 sy 8.875
        ('gen_tw_65', 'gen_area', ('tw_65',), 84, 82, 65, 8, 1.5),   # 65x8 tex 320 sx 4.938 sy 8.750
        ('rows_64x64', 'rows', ('carry', 'chunked', 'many_passes', 'th_64', 'tw_64'), 161, 82, 64, 64, 1.5),   # 64x64 tex 320 sx 3.875 sy 3.875
        ('gen_65x64', 'gen_area', ('th_64', 'tw_65'), 8, 152, 65, 64, 1.5),   # 65x64 tex 320 sx 3.846 sy 3.859
        ('rot_64x65', 'rot', ('th_65', 'tw_64'), 85, 152, 64, 65, 1.5),   # 64x65 tex 320 sx 3.859 sy 3.846
        ('gen_65x65', 'gen_area', ('th_65', 'tw_65'), 161, 152, 65, 65, 1.5),   # 65x65 tex 320 sx 3.815 sy 3.815
        ('rows_chunked_12', 'rows', ('carry', 'chunked', 'many_passes'), 238, 152, 12, 20, 3.5),   # 12x20 tex 229 sx 12.083 sy 10.600
        ('rows_61x63', 'rows', ('chunked', 'many_passes'), 8, 223, 61, 63, 1.5),   # 61x63 tex 320 sx 4.016 sy 4.000
        ('rows_thin_8_flip', 'rows', ('carry', 'flip'), 330, 10, 0, 8, 1.5),   # 3x8 tex 229 sx 10.667 sy 28.625
        ('rows_vertical_20_flip', 'rows', ('flip',), 350, 10, 0, 20, 1.5),   # 3x20 tex 320 sx 10.667 sy 16.000
        ('rot_int_flip', 'rot_int', ('flip',), 370, 10, 0, 40, 2.5),   # 4x40 tex 320 sx 8.000 sy 8.000
        ('rows_th_64_flip', 'rows', ('carry', 'chunked', 'flip', 'many_passes', 'th_64'), 390, 10, 12, 64, 1.5),   # 12x64 tex 320 sx 7.500 sy 5.000
        ('rot_th_65_flip', 'rot', ('flip', 'th_65'), 414, 10, 12, 65, 1.5),   # 12x65 tex 320 sx 7.417 sy 4.923
        ('rows_tw_64_flip', 'rows', ('carry', 'chunked', 'flip', 'many_passes', 'tw_64'), 438, 10, 64, 8, 2.5),   # 64x8 tex 320 sx 5.016 sy 8.875
        ('gen_tw_65_flip', 'gen_area', ('flip', 'tw_65'), 514, 10, 65, 8, 2.5),   # 65x8 tex 320 sx 4.938 sy 8.750
        ('rows_64x64_flip', 'rows', ('carry', 'chunked', 'flip', 'many_passes', 'th_64', 'tw_64'), 330, 81, 64, 64, 2.5),   # 64x64 tex 320 sx 3.875 sy 3.875
        ('gen_65x64_flip', 'gen_area', ('flip', 'th_64', 'tw_65'), 406, 81, 65, 64, 2.5),   # 65x64 tex 320 sx 3.846 sy 3.859
        ('rot_64x65_flip', 'rot', ('flip', 'th_65', 'tw_64'), 483, 81, 64, 65, 3.5),   # 64x65 tex 320 sx 3.859 sy 3.846
        ('rows_upward', 'rows', ('carry', 'chunked', 'flip', 'many_passes'), 559, 111, 10, -30, 2.5),   # 10x30 tex 320 sx 13.100 sy 10.433
        ('left_rows', 'rows', ('chunked', 'many_passes'), -3, 300, 8, 40, 2.5),   # 8x40 tex 320 sx 11.750 sy 8.000
        ('left_rot', 'rot', (), -2, 350, 3, 70, 1.5),   # 3x70 tex 320 sx 15.000 sy 4.586
        ('top_rows', 'rows', ('carry',), 286, -5, 3, 30, 2.5),   # 4x30 tex 320 sx 15.750 sy 10.700
        ('top_rot_int', 'rot_int', (), 300, -8, 0, 32, 2.5),   # 4x32 tex 320 sx 8.000 sy 10.000
        ('right_rows', 'rows', ('carry', 'chunked', 'flip', 'many_passes'), 636, 300, 10, 40, 2.5),   # 10x40 tex 320 sx 10.800 sy 7.950
        ('right_gen', 'gen_area', ('flip', 'tw_65'), 600, 360, 65, 8, 2.5),   # 65x8 tex 320 sx 4.938 sy 8.750
        ('bottom_rows', 'rows', ('carry',), 300, 470, 4, 30, 2.5),   # 4x30 tex 320 sx 18.500 sy 10.700
        ('bottom_rot', 'rot', ('flip',), 340, 440, 0, 66, 1.5),   # 3x66 tex 320 sx 10.667 sy 4.848
        ('corner_rows', 'rows', ('carry', 'chunked', 'flip', 'many_passes'), 630, 460, 20, 30, 2.5),   # 20x30 tex 320 sx 10.200 sy 9.467
        # a streak that starts outside the frame and ends inside it: the tile is placed at its start and nothing of it is seen
        ('skipped_right', 'skipped', (), 645, 100, -15, 40, 2.5),   # 15x40 tex 320 sx 9.467 sy 7.750
        ('skipped_bottom', 'skipped', (), 100, 485, 0, -40, 2.5),   # 4x40 tex 320 sx 8.000 sy 8.000
    ],
    # long streaks: scale_x around 2 and below it, RS_LINEAR (longer than the texture), TW_MAX once more
    'long': [
        ('rot_sx_2.016', 'rot', ('sx_at_2',), 8, 10, 61, 200, 1.5),   # 61x200 tex 320 sx 2.016 sy 1.575
        ('rot_sx_2.000_tw_64', 'rot', ('sx_at_2', 'tw_64'), 81, 10, 64, 200, 2.5),   # 64x200 tex 320 sx 2.000 sy 1.570
        ('gen_sx_1.985_tw_65', 'gen_area', ('sx_below_2', 'tw_65'), 157, 10, 65, 200, 2.5),   # 65x200 tex 320 sx 1.985 sy 1.570
        ('rot_sx_below_2', 'rot', ('sx_below_2',), 234, 10, 40, 300, 2.5),   # 40x300 tex 320 sx 1.850 sy 1.070
        ('rot_sx_1.5_tw_64', 'rot', ('sx_below_2', 'tw_64'), 8, 316, 64, 300, 2.5),   # 64x300 tex 320 sx 1.531 sy 1.063
        ('gen_area_wide', 'gen_area', ('sx_below_2',), 84, 316, 120, 160, 1.5),   # 120x160 tex 320 sx 1.808 sy 1.719
        ('gen_linear_vertical', 'gen_linear', (), 216, 316, 0, 330, 2.5),   # 4x330 tex 320 sx 8.000 sy 0.970
        ('gen_linear_sx_2', 'gen_linear', ('sx_at_2',), 266, 316, -30, 330, 1.5),   # 30x330 tex 320 sx 2.000 sy 0.973
        ('rot_sx_2_flip', 'rot', ('flip', 'sx_at_2'), 330, 10, 61, 200, 1.5),   # 61x200 tex 320 sx 2.016 sy 1.575
        ('gen_linear_tw_64_flip', 'gen_linear', ('flip', 'sx_below_2', 'tw_64'), 403, 10, 64, 330, 1.5),   # 64x330 tex 320 sx 1.438 sy 0.970
        ('gen_linear_tw_65_flip', 'gen_linear', ('flip', 'sx_below_2', 'tw_65'), 479, 10, 65, 330, 1.5),   # 65x330 tex 320 sx 1.431 sy 0.970
        ('rot_int_3x2_flip', 'rot_int', ('flip',), 586, 10, -30, 160, 3.5),   # 30x160 tex 320 sx 3.000 sy 2.000
        ('gen_linear_flip', 'gen_linear', ('flip',), 550, 10, 0, 330, 1.5),   # 3x330 tex 320 sx 10.667 sy 0.970
        ('rot_tall_flip', 'rot', ('flip',), 572, 20, 3, 300, 1.5),   # 3x300 tex 320 sx 11.667 sy 1.067
        ('left_gen_linear', 'gen_linear', (), -2, 100, 6, 330, 2.5),   # 6x330 tex 320 sx 6.167 sy 0.970
        ('top_rot', 'rot', ('flip', 'sx_below_2'), 284, -20, 40, 300, 2.5),   # 40x300 tex 320 sx 1.850 sy 1.070
        ('bottom_gen_linear', 'gen_linear', ('flip',), 560, 200, 0, 330, 2.5),   # 4x330 tex 320 sx 8.000 sy 0.970
        ('right_rot', 'rot', ('flip',), 620, 20, 40, 150, 2.5),   # 40x150 tex 320 sx 2.825 sy 2.113
    ],
    # Big drops: BIG_ROWS_MAX_PX from both sides, blocks (tw > bw0 = min(1024 / min(16, th), tw)), one wave, one row, one column
    'big': [
        ('big_lds_thin', 'big_lds', (), 8, 10, 0, 20, 5.0),   # 5x20 tex 114
        ('big_lds_15x40', 'big_lds', (), 28, 10, 10, 40, 5.0),   # 15x40 tex 229
        ('big_one_wave_8x8', 'big_lds', ('big_one_wave',), 50, 10, 3, 8, 5.0),   # 8x8 tex 80
        ('big_one_row', 'big_lds', ('big_one_wave', 'th_1'), 70, 10, 0, 1, 5.0),   # 5x1 tex 80
        ('big_lds_64x128', 'big_lds', ('big_px_le_8192',), 90, 10, 59, 128, 5.0),   # 64x128 tex 320: 8192 pixels
        ('big_65x128', 'big', ('big_blocks', 'big_px_gt_8192'), 161, 10, 60, 128, 5.0),   # 65x128 tex 320: 8320
        ('big_lds_64x127', 'big_lds', ('big_px_le_8192',), 233, 10, 59, 127, 5.0),   # 64x127 tex 320
        ('big_64x129', 'big', ('big_px_gt_8192',), 8, 144, 59, 129, 5.0),   # 64x129 tex 320: 8256
        ('big_lds_blocks_91x90', 'big_lds', ('big_blocks', 'big_px_le_8192'), 79, 144, 86, 90, 5.0),   # 91x90 tex 320: 8190
        ('big_lds_border', 'big_lds', ('big_border',), 177, 144, 30, 200, 6.0),   # 36x200 tex 320
        ('big_lds_205x8', 'big_lds', ('big_blocks',), 330, 10, 200, 8, 5.0),   # 205x8 tex 320: bw0 = 128
        ('big_lds_210x39', 'big_lds', ('big_blocks', 'big_px_le_8192'), 330, 24, 205, 39, 5.0),   # 210x39 tex 320: 8190
        ('big_210x40', 'big', ('big_blocks', 'big_px_gt_8192'), 330, 69, 205, 40, 5.0),   # 210x40 tex 320: 8400
        ('big_105x300', 'big', ('big_blocks', 'big_border'), 330, 115, 100, 300, 5.0),   # 105x300 tex 320
        ('big_26x320', 'big', ('big_border', 'big_px_gt_8192'), 442, 115, 20, 320, 6.0),   # 26x320 tex 320: 8320
        ('big_lds_leaning_left', 'big_lds', (), 514, 115, -40, 60, 5.0),   # 45x60 tex 320
        ('big_lds_upward', 'big_lds', (), 526, 145, 10, -30, 5.0),   # 15x30 tex 160
        ('right_big_tw_1', 'big_lds', ('big_one_wave', 'tw_1'), 639, 100, 0, 30, 5.0),   # 1x30 tex 160
        ('right_big_tw_2', 'big_lds', ('big_one_wave',), 638, 140, 0, 30, 5.0),   # 2x30 tex 160
        ('right_big_tall', 'big_lds', (), 636, 180, 0, 200, 5.0),   # 4x200 tex 320
        ('left_big', 'big_lds', (), 0, 100, -3, 30, 5.0),   # 5x30 tex 160
        ('bottom_big', 'big_lds', (), 300, 470, 10, 30, 5.0),   # 15x10 tex 160
        ('top_big', 'big_lds', (), 300, 5, 10, -30, 5.0),   # 15x5 tex 160
        ('bottom_right_big', 'big_lds', (), 600, 400, 100, 150, 5.0),   # 40x80 tex 320
    ],
}
FAMILIES = tuple(CATALOGUE)

# One database per side of a texture limit: (name, tex_heights, tex_width, the route every drop must take, drops as (x0, y0, dx,
# dy, image width)).  The limit's height comes first: DBManager.texture_bucket gives a drop whose width / length is below the
# first texture's width / height that texture, and every drop here is that thin.
_ROT_LIMIT_DROPS = ((20, 20, 0, 40, 1.5), (60, 20, 12, 64, 1.5), (100, 20, 64, 8, 1.5), (200, 20, 3, 20, 1.5), (400, 60, 10, -30, 2.5),
                    (450, 20, 61, 63, 1.5))
_BIG_LIMIT_DROPS = ((20, 20, 0, 40, 5.0), (60, 20, 10, 60, 5.0), (100, 20, 59, 128, 5.0), (200, 20, 30, 200, 6.0), (400, 20, 200, 30, 5.0),
                    (20, 250, 3, 36, 5.0))
TEXTURE_LIMIT_DBS = [
    ('pair_fits_321', (321, 160, 120, 100, 80), 32, 'rows', _ROT_LIMIT_DROPS),       # pair_bytes = 24624 <= RW_PAIR_BYTES
    ('pair_over_322', (322, 160, 120, 100, 80), 32, 'rot', _ROT_LIMIT_DROPS),        # 24704: k_tile
    ('tex_lds_fits_323', (323, 160, 120, 100, 80), 32, 'rot', _ROT_LIMIT_DROPS),     # (323 + 4) * 36 = 11772 <= TEX_LDS
    ('tex_lds_over_324', (324, 160, 120, 100, 80), 32, 'gen_area', _ROT_LIMIT_DROPS),    # 11808; the 64 x 8 drop has nW = 325 > RW_NW
    ('big_fits_357', (357, 160, 120, 100, 80), 64, 'big_lds', _BIG_LIMIT_DROPS),     # (357 + 4) * 68 + 48 = 24596 <= RW_PAIR_BYTES
    ('big_over_358', (358, 160, 120, 100, 80), 64, 'big', _BIG_LIMIT_DROPS),         # 24664
]
# and one the default database cannot reach: tile_is_rows' scale_x >= 2 on tiles of at most 64 rows needs a short texture.
# (name, route, flags, drop): 48 x 40 has scale_x = 97 / 48, 49 x 40 has 97 / 49
SCALE_X_DB = ('scale_x_2', (100, 90, 80, 70, 60), 32, [
    ('rows_sx_2.087', 'rows', ('carry', 'chunked', 'many_passes', 'sx_at_2'), (100, 20, 46, 40, 2.5)),
    ('rows_sx_2.021', 'rows', ('carry', 'chunked', 'many_passes', 'sx_at_2'), (180, 20, 48, 40, 2.5)),
    ('rot_sx_1.980', 'rot', ('sx_below_2',), (260, 20, 49, 40, 2.5)),
    ('rot_sx_1.960_flip', 'rot', ('flip', 'sx_below_2'), (340, 20, 50, 40, 2.5)),
    ('rows_sx_2.159', 'rows', ('carry', 'chunked', 'many_passes'), (20, 20, 44, 40, 2.5)),
    ('rows_sx_2.970_flip', 'rows', ('carry', 'chunked', 'flip', 'many_passes'), (340, 100, 33, 26, 2.5)),
])

# The batches of the list-scheduling cases (k_lists' histogram, k_rows_scatter, k_rows_shares, the share counter, the texture
# switch of k_tile_rows): name -> the frames of one call, each a list of drops (x0, y0, dx, dy, image width), [] an empty
# frame, or the name of a catalogue family.  'one_texture': every drop is given the first drop's texture, so that the whole
# frame is one bucket of the batch-wide list (and all forty raw tiles are one: k_dedup).
_FORTY = [(8 + 15 * k, 50, 3, 20, 1.5) for k in range(40)]
LIST_SHAPES = {
    'only_big': dict(frames=[[e[3:] for e in CATALOGUE['big'][:12]]]),
    'only_rot_int': dict(frames=[[(20 + 30 * k, 30, 0, 40, 2.5) for k in range(8)]]),          # no rows tile in the call
    'one_rows_tile': dict(frames=[[(100, 100, 12, 64, 1.5)]]),
    'three_rows_tiles': dict(frames=[[(100, 100, 12, 64, 1.5), (200, 100, 0, 20, 1.5), (400, 100, 64, 8, 1.5)]]),    # fewer than any share count
    'forty_copies': dict(frames=[_FORTY], one_texture=True),
    'empty_catalogue_empty': dict(frames=[[], 'small', []]),
}


def particle(k, drop, H=CAT_H, W=CAT_W, cam=h.KITTI):
    x0, y0, dx, dy, iw = drop
    return h.streak(k, x0, y0, x0 + dx, y0 + dy, iw, iw, 6.0, H, W, cam)


def particles(drops, H=CAT_H, W=CAT_W, cam=h.KITTI):
    return [particle(k, d, H, W, cam) for k, d in enumerate(drops)]


def catalogue_particles(family):
    return particles([e[3:] for e in CATALOGUE[family]])


def scene(tmp, drops, **db):
    """One 480 x 640 KITTI frame with these drops (and, with tex_heights / tex_width, another database)."""
    return h.Scene(tmp, CAT_H, CAT_W, 0, frames=[dict(id=0, t=2000, d=0, drops=particles(drops))], **db)


def raw_tile_keys(sc, drops):
    """(keys n x 8 uint32, live) of a frame's drops: rr_device.h raw_tile_key, what k_dedup compares."""
    plans, _ = h.emu_plan(sc, drops)
    keys = np.zeros((max(len(drops), 1), 8), np.uint32)
    h.hostemu().emu_raw_tile_keys(h._p(np.ascontiguousarray(drops)), len(drops), h._p(plans), h._p(keys))
    live = (plans['status'] == RR_DROP_OK) & (plans['vis_w'] > 0) & (plans['vis_h'] > 0)
    return keys[:len(drops)], live


def expected_shared(sc, frames):
    """rr_batch_counts [7] summed over a call of these frames' drops with RR_OPT_DEDUP 1: the live drops less their distinct
    raw-tile keys (one drop per key renders the tile, whichever frame it is in)."""
    n_live, distinct = 0, set()
    for drops in frames:
        if len(drops):
            keys, live = raw_tile_keys(sc, drops)
            n_live += int(live.sum())
            distinct |= {keys[i].tobytes() for i in np.nonzero(live)[0]}
    return n_live - len(distinct)


def frame_drops(sc, n):
    """The frame's packed drops; nothing may have been filtered (drop i is entry i)."""
    drops = sc.product_drops(0)
    assert len(drops) == n, (len(drops), n)
    return drops
