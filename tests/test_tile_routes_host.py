"""CPU tier of the raw-tile routes (tests/tile_routes.py): the census -- every catalogue entry takes the route and carries the
flags written beside it, every route and flag is reached, every texture-limit database sits on its side -- the g++ build of the
kernel arithmetic against the numpy oracle on the catalogue frames, the kernels' own row_interval / tile_pitch inside the row-walk
emulation (a sample outside the interval or an interval longer than the pitch is an error), and the lane-by-lane emulation of
big_tile, the Big path of k_tile_rows, against warp_big_pixel.  The GPU tier is tests/test_gpu_tile_routes.py."""

import numpy as np
import pytest

import helpers as h
import tile_routes as tr


@pytest.fixture(scope='module')
def catalogue(tmp_path_factory):
    """family -> (scene, drops, records)."""
    out = {}
    for fam in tr.FAMILIES:
        sc = tr.scene(tmp_path_factory.mktemp(fam), [e[3:] for e in tr.CATALOGUE[fam]])
        drops = tr.frame_drops(sc, len(tr.CATALOGUE[fam]))
        out[fam] = (sc, drops, tr.classify_drops(sc, drops))
    return out


# ---------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('fam', tr.FAMILIES)
def test_catalogue_entries_take_their_route(catalogue, fam):
    """A threshold that moves names the entries it moved."""
    _, _, recs = catalogue[fam]
    bad = [(e[0], e[1], sorted(e[2]), '->', r['route'], sorted(r['flags']), {k: r[k] for k in ('tex_h', 'tex_w', 'tw', 'th', 'nW', 'nH', 'scale_x', 'bw0')})
           for e, r in zip(tr.CATALOGUE[fam], recs) if r['route'] != e[1] or r['flags'] != set(e[2])]
    assert not bad, bad
    assert len(recs) <= 60
    live = [r for r in recs if r['live']]
    assert all(r['live'] == (r['route'] != 'skipped') for r in recs)
    for a in live:                                           # no two footprints overlap: a differing pixel belongs to one entry
        for b in live:
            if a['i'] < b['i']:
                ax0, ay0, ax1, ay1 = a['box']
                bx0, by0, bx1, by1 = b['box']
                assert not (ax0 < bx1 and bx0 < ax1 and ay0 < by1 and by0 < ay1), (tr.CATALOGUE[fam][a['i']][0], tr.CATALOGUE[fam][b['i']][0])


def test_catalogue_reaches_every_route_and_flag(catalogue):
    total = {k: 0 for k in tr.ROUTES + tr.FLAGS}
    print('\n%-16s' % 'route / flag' + ''.join('%8s' % f for f in tr.FAMILIES))
    per = {f: tr.census(catalogue[f][2]) for f in tr.FAMILIES}
    for k in total:
        total[k] = sum(per[f][k] for f in tr.FAMILIES)
        print('%-16s' % k + ''.join('%8d' % per[f][k] for f in tr.FAMILIES))
    lost = [k for k, v in total.items() if v == 0]
    assert not lost, 'no catalogue entry reaches: %s' % lost
    # every family has entries on each frame border, and the rotate families one that the border crops
    for f in tr.FAMILIES:
        live = [r for r in catalogue[f][2] if r['live']]
        assert min(r['box'][0] for r in live) == 0 and min(r['box'][1] for r in live) == 0, f
        assert max(r['box'][2] for r in live) == tr.CAT_W and max(r['box'][3] for r in live) == tr.CAT_H, f
        if f != 'big':                                       # (a Big tile is sized to what the frame holds of it)
            for side, wh, size in ((0, 2, 'tw'), (1, 3, 'th')):
                assert any(r['box'][side] == 0 and r[size] > r['box'][wh] - r['box'][side] for r in live), (f, side)
                assert any(r['box'][wh] == (tr.CAT_W, tr.CAT_H)[side] and r[size] > r['box'][wh] - r['box'][side] for r in live), (f, side)


def test_thresholds_side_by_side(catalogue):
    """Both sides of each threshold, by entry: the values the routes are decided on."""
    by = {e[0]: r for f in tr.FAMILIES for e, r in zip(tr.CATALOGUE[f], catalogue[f][2])}
    lim = tr.limits()
    assert (lim['TW_MAX'], lim['BIG_ROWS_MAX_PX']) == (64, 8192)        # the values the entries' names carry
    v = lambda name, *keys: tuple(by[name][k] for k in keys)
    # tile_is_rows: th <= 64 (the vertical spans travel by lane shuffles), else k_tile
    assert v('rows_th_64', 'route', 'th') == ('rows', 64) and v('rot_th_65', 'route', 'th') == ('rot', 65)
    assert v('rows_th_64_oblique', 'route', 'th') == ('rows', 64) and v('rot_th_65_oblique', 'route', 'th') == ('rot', 65)
    assert v('rot_int_th_64', 'route', 'th') == ('rot_int', 64)        # integer ratios never take the row walk
    # tw <= 64 = TW_MAX: past it neither k_tile_rows nor k_tile
    assert v('rows_tw_64', 'route', 'tw') == ('rows', 64) and v('gen_tw_65', 'route', 'tw') == ('gen_area', 65)
    assert [v(n, 'route', 'tw', 'th') for n in ('rows_64x64', 'gen_65x64', 'rot_64x65', 'gen_65x65')] == [
        ('rows', 64, 64), ('gen_area', 65, 64), ('rot', 64, 65), ('gen_area', 65, 65)]
    # scale_x around 2 on the default database (tiles taller than 64 rows: k_tile either side; SCALE_X_DB has the rows side)
    assert by['rot_sx_2.000_tw_64']['scale_x'] == 2.0 and 1.98 < by['gen_sx_1.985_tw_65']['scale_x'] < 2.0 < by['rot_sx_2.016']['scale_x'] < 2.02
    assert by['gen_linear_vertical']['scale_y'] < 1.0 <= by['rot_tall_flip']['scale_y']
    # Big: BIG_ROWS_MAX_PX pixels is the last tile of k_tile_rows, whatever its shape
    px = lambda n: by[n]['tw'] * by[n]['th']
    assert [(px(n), by[n]['route']) for n in ('big_lds_64x128', 'big_65x128', 'big_64x129', 'big_lds_blocks_91x90', 'big_lds_210x39', 'big_210x40', 'big_26x320')] == [
        (8192, 'big_lds'), (8320, 'big'), (8256, 'big'), (8190, 'big_lds'), (8190, 'big_lds'), (8400, 'big'), (8320, 'big')]
    assert v('right_big_tw_1', 'tw', 'th') == (1, 30) and v('big_one_row', 'tw', 'th') == (5, 1)
    assert by['big_lds_205x8']['bw0'] == 128 and by['big_65x128']['bw0'] == 64
    # pass shapes of the row walk: one row per lane; segments of cells; the narrowest passes (4 rows of 16 segments)
    assert v('rows_vertical_20', 'R', 'NS') == (64, 1) and v('rows_chunked_12', 'R', 'NS') == (21, 3) and v('rows_64x64', 'R', 'NS', 'passes') == (4, 16, 62)


@pytest.mark.parametrize('tile_rows', [0, 1])
def test_routes_without_the_row_walk(catalogue, tile_rows):
    """RR_OPT_TILE_ROWS 0 / 1: a rows tile falls to k_tile (all of them fit it here), a Big tile to k_tile_big."""
    for fam in tr.FAMILIES:
        for e, r in zip(tr.CATALOGUE[fam], catalogue[fam][2]):
            got = r['routes'][tile_rows]
            if e[1] == 'rows':
                assert got == ('rot' if tile_rows == 0 else 'rows'), e[0]
            elif e[1] == 'big_lds':
                assert got == 'big', e[0]
            else:
                assert got == e[1], e[0]


def _pair_bytes(sh, sw):
    q = sw + 4
    while q & 3 != 2:
        q += 1
    return ((sh + 3) * q * 2 + 15) & ~15


def test_texture_limit_databases_sit_on_their_side(tmp_path):
    lim = tr.limits()
    # the heights are the last that fits and the first that does not, by the limits' own arithmetic
    assert _pair_bytes(321, 32) <= lim['RW_PAIR_BYTES'] < _pair_bytes(322, 32)
    assert (323 + 4) * 36 <= lim['TEX_LDS'] < (324 + 4) * 36
    assert (357 + 4) * 68 + 48 <= lim['RW_PAIR_BYTES'] < (358 + 4) * 68 + 48
    for name, heights, width, route, drops in tr.TEXTURE_LIMIT_DBS:
        sc = tr.scene(tmp_path / name, drops, tex_heights=heights, tex_width=width)
        recs = tr.classify_drops(sc, tr.frame_drops(sc, len(drops)))
        assert len(recs) >= 6
        assert [(r['route'], r['tex_h'], r['tex_w']) for r in recs] == [(route, heights[0], width)] * len(recs), name
        if name == 'tex_lds_over_324':
            assert max(r['nW'] for r in recs) > lim['RW_NW']
    name, heights, width, entries = tr.SCALE_X_DB
    sc = tr.scene(tmp_path / name, [e[3] for e in entries], tex_heights=heights, tex_width=width)
    recs = tr.classify_drops(sc, tr.frame_drops(sc, len(entries)))
    bad = [(e[0], r['route'], sorted(r['flags']), r['scale_x']) for e, r in zip(entries, recs) if r['route'] != e[1] or r['flags'] != set(e[2]) or r['th'] > 64]
    assert not bad, bad
    sx = {e[0]: r['scale_x'] for e, r in zip(entries, recs)}
    assert sx['rot_sx_1.980'] < 2.0 <= sx['rows_sx_2.021'] < 2.03


def test_sharing_cases_by_raw_tile_key(catalogue, tmp_path):
    """What the GPU tier's sharing test rests on: no two entries of the 'small' frame have one raw tile (so the frame twice
    shares exactly its live drops), and forty shifted copies of a streak with one texture are two tiles (plain and mirrored)."""
    sc, drops, recs = catalogue['small']
    assert tr.expected_shared(sc, [drops]) == 0
    assert tr.expected_shared(sc, [drops, drops]) == sum(r['live'] for r in recs)
    forty = tr.LIST_SHAPES['forty_copies']['frames'][0]
    sc = tr.scene(tmp_path, forty)
    drops = tr.frame_drops(sc, 40)
    drops['tex_index'] = drops['tex_index'][0]
    recs = tr.classify_drops(sc, drops)
    assert {r['route'] for r in recs} == {'rows'} and len({r['tex'] for r in recs}) == 1
    assert tr.expected_shared(sc, [drops]) == 38


def test_list_shapes_hold_what_they_say(tmp_path):
    for name, shape in tr.LIST_SHAPES.items():
        for k, fr in enumerate(shape['frames']):
            if isinstance(fr, str) or not fr:
                continue
            sc = tr.scene(tmp_path / name / str(k), fr)
            routes = {r['route'] for r in tr.classify_drops(sc, tr.frame_drops(sc, len(fr)))}
            want = {'only_big': {'big_lds', 'big'}, 'only_rot_int': {'rot_int'}}.get(name, {'rows'})
            assert routes == want, (name, routes)


# ---------------------------------------------------------------------------
# oracle against host build
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('fam', tr.FAMILIES)
def test_hostemu_matches_oracle_on_catalogue(catalogue, fam):
    sc, drops, recs = catalogue[fam]
    bg, env = sc.frame_inputs(0)
    emu = h.emu_render(sc, bg, bg, env, drops)
    ref = h.oracle_render(sc, 0, bg, bg, env, faithful=False)
    tr.check(emu, ref, recs, fam)
    assert emu['mask'].max() > 0
    for e, r in zip(tr.CATALOGUE[fam], recs):                # every live entry leaves a mark of its own
        if r['live']:
            x0, y0, x1, y1 = r['box']
            assert emu['mask'][y0:y1, x0:x1].max() > 0, e[0]


# ---------------------------------------------------------------------------
# the kernels' interval in the row-walk emulation
# ---------------------------------------------------------------------------
def _walk(plan, db, buf=344):
    """emu_tile_rows_mode with the kernel's row_interval; -1: not a plan the row walk takes."""
    texels, hs, ws, offs = db
    n = max(int(plan['tw']) * int(plan['th']), 1)
    out, ref = np.full(n, -1.0), np.full(n, -2.0)
    p = np.array([plan], dtype=h.PLAN_DTYPE)
    return h.hostemu().emu_tile_rows_mode(h._p(p), h._p(texels), h._p(hs), h._p(ws), h._p(offs), int(buf), h._p(out), h._p(ref), 1)


def _interval(plan, db):
    texels, hs, ws, offs = db
    p = np.array([plan], dtype=h.PLAN_DTYPE)
    return h.hostemu().emu_row_interval_check(h._p(p), h._p(texels), h._p(hs), h._p(ws), h._p(offs))


def test_kernel_interval_on_catalogue(catalogue, tmp_path):
    walked = checked = 0
    cases = [(catalogue[f][0], catalogue[f][1], catalogue[f][2]) for f in ('small', 'long')]
    name, heights, width, entries = tr.SCALE_X_DB
    sc = tr.scene(tmp_path, [e[3] for e in entries], tex_heights=heights, tex_width=width)
    drops = tr.frame_drops(sc, len(entries))
    cases.append((sc, drops, tr.classify_drops(sc, drops)))
    for sc, drops, recs in cases:
        plans, _ = h.emu_plan(sc, drops)
        db = tr.db_arrays(sc)
        for r in recs:
            if r['route'] not in ('rows', 'rot'):
                continue
            assert _interval(plans[r['i']], db) == 0, r
            checked += 1
            rc = _walk(plans[r['i']], db)
            assert rc == 0 if r['route'] == 'rows' else rc in (0, -1), (rc, r)
            walked += rc == 0
    assert checked >= 40 and walked >= 30, (checked, walked)


def test_kernel_interval_on_a_kitti_scene(tmp_path):
    """The scene of tests/test_tile_rows_host.py, every rotate tile: the walk over row_interval's columns gives the definition's
    bits, with the kernel's buffer and with one that forces column chunks."""
    H, W = 375, 1242
    sc = h.Scene(tmp_path, H, W, 1400, cam=h.KITTI, seed0=3000)
    drops = sc.product_drops(0)
    plans, sizes = h.emu_plan(sc, drops)
    db = tr.db_arrays(sc)
    taken = 0
    for k in range(len(plans)):
        if plans[k]['status'] != 0 or sizes[k] == 0 or plans[k]['kind'] != tr.KIND_ROT:
            continue
        assert _interval(plans[k], db) == 0, k
        for buf in (344, 96):
            rc = _walk(plans[k], db, buf)
            assert rc in (0, -1), (k, buf, rc, plans[k]['tw'], plans[k]['th'], plans[k]['nW'], plans[k]['nH'])
            taken += rc == 0
    assert taken > 600, taken


def test_kernel_interval_on_awkward_scales(tmp_path):
    """The sweep of tests/test_tile_rows_host.py (output sizes that put scale_x on integers, a hair off them and near 2)."""
    H, W = 375, 1242
    sc = h.Scene(tmp_path, H, W, 300, cam=h.KITTI, seed0=3100)
    plans, sizes = h.emu_plan(sc, sc.product_drops(0))
    db = tr.db_arrays(sc)
    rot = [k for k in range(len(plans)) if plans[k]['status'] == 0 and sizes[k] > 0 and plans[k]['kind'] == tr.KIND_ROT]
    done = 0
    for k in rot[:40]:
        nW, nH = int(plans[k]['nW']), int(plans[k]['nH'])
        for tw in sorted(set([1, 2, 3, 5, 7, nW // 8, nW // 4, nW // 3, nW // 2, nW // 2 - 1, 31, 47, 64])):
            for th in (1, 2, 3, 9, nH // 7, nH // 2, nH - 1):
                if tw < 1 or th < 1 or tw > 64 or th > nH:
                    continue
                q = plans[k].copy()
                q['tw'], q['th'] = tw, th
                q['inv_sx'], q['inv_sy'] = tw / nW, th / nH
                q['scale_x'], q['scale_y'] = 1.0 / q['inv_sx'], 1.0 / q['inv_sy']
                if q['scale_x'] < 1 or q['scale_y'] < 1:
                    continue
                eps = 2.220446049250313e-16
                q['rs_mode'] = 1 if abs(q['scale_x'] - round(float(q['scale_x']))) < eps and abs(q['scale_y'] - round(float(q['scale_y']))) < eps else 0
                rc = _walk(q, db)
                assert rc in (0, -1), (k, tw, th, nW, nH, rc)
                done += rc == 0
    assert done > 1500, done


ANGLES = [0.0, 0.01, -0.01, 45.0, -45.0, 89.99, -89.99, 90.0, -90.0, 180.0,
          1e-7, -1e-7, 3e-8, -3e-8, 90.0 - 1e-7, 90.0 + 1e-7, 90.0 - 3e-8, 90.0 + 3e-8]     # the last eight: |ma| * 1024 on both sides of 1e-6


def test_kernel_interval_over_rotation_angles(tmp_path):
    """row_geom treats an axis whose coefficient |ma[0]|, |ma[3]| * 1024 is below 1e-6 as constant along the row: angles at
    which the coefficients vanish, nearly vanish and cross that test, on a tall and a short texture, narrow and wide tiles."""
    base = [(20, 20, 3, 20, 1.5), (100, 20, 12, 20, 1.5), (200, 20, 0, 8, 3.5), (300, 20, 12, 20, 3.5)]
    sc = tr.scene(tmp_path, base)
    drops0 = tr.frame_drops(sc, len(base))
    db = tr.db_arrays(sc)
    walked, below = 0, 0
    for deg in ANGLES:
        drops = drops0.copy()
        drops['rot_cos'], drops['rot_sin'] = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
        plans, _ = h.emu_plan(sc, drops)
        for k in range(len(plans)):
            p = plans[k]
            assert p['status'] == 0 and p['kind'] == tr.KIND_ROT
            below += int(min(abs(p['ma'][0]), abs(p['ma'][3])) * 1024.0 < 1e-6)
            assert _interval(p, db) == 0, (deg, k, p['ma'])
            rc = _walk(p, db)
            assert rc in (0, -1), (deg, k, rc, p['tw'], p['th'], p['nW'], p['nH'])
            walked += rc == 0
    assert walked >= 3 * len(ANGLES) and 16 <= below < 4 * len(ANGLES), (walked, below)


# ---------------------------------------------------------------------------
# big_tile, lane by lane
# ---------------------------------------------------------------------------
def _big(plan, db):
    """(return code, the emulation's tile, the definition's)."""
    texels, hs, ws, offs = db
    n = max(int(plan['tw']) * int(plan['th']), 1)
    out, ref = np.full(n, -1.0), np.full(n, -2.0)
    p = np.array([plan], dtype=h.PLAN_DTYPE)
    rc = h.hostemu().emu_big_lds(h._p(p), h._p(texels), h._p(hs), h._p(ws), h._p(offs), len(hs), h._p(out), h._p(ref))
    return rc, out, ref


def test_big_tile_emulation_on_catalogue(catalogue):
    sc, drops, recs = catalogue['big']
    plans, _ = h.emu_plan(sc, drops)
    db = tr.db_arrays(sc)
    seen = set()
    for e, r in zip(tr.CATALOGUE['big'], recs):
        rc, out, ref = _big(plans[r['i']], db)
        assert rc == (0 if r['route'] == 'big_lds' else -1), (e[0], rc)
        if rc == 0:
            assert out.max() > 0, e[0]
            seen |= r['flags']
    assert {'big_blocks', 'big_border', 'big_one_wave', 'tw_1', 'th_1', 'big_px_le_8192'} <= seen


def test_big_tile_emulation_on_a_nuscenes_scene(tmp_path):
    H, W = 450, 800
    sc = h.Scene(tmp_path, H, W, 1500, cam=h.NUSCENES, seed0=6100, far_fraction=0.2)
    drops = sc.product_drops(0)
    plans, sizes = h.emu_plan(sc, drops)
    db = tr.db_arrays(sc)
    taken = blocks = 0
    for k in range(len(plans)):
        if plans[k]['status'] != 0 or sizes[k] == 0 or plans[k]['kind'] != tr.KIND_BIG:
            continue
        rc, _, _ = _big(plans[k], db)
        assert rc in (0, -1), (k, rc, plans[k]['tw'], plans[k]['th'])
        taken += rc == 0
        blocks += rc == 0 and plans[k]['tw'] > plans[k]['bw0']
    assert taken >= 20, (taken, blocks)


def _hand_plan(base, tw, th, mi):
    q = base.copy()
    q['tw'], q['th'] = tw, th
    q['bw0'] = min(1024 // min(16, th), tw)                  # plan_drop
    q['mi'] = np.asarray(mi, np.float64).reshape(9)
    return q


def test_big_tile_emulation_on_hand_made_homographies(catalogue):
    """Plans whose inverse homography is written by hand, so that the 4 x 4 windows sit where the kernel's clamps, its
    aligned-pair fetch and its division by tw can go wrong."""
    sc, drops, recs = catalogue['big']
    plans, _ = h.emu_plan(sc, drops)
    db = tr.db_arrays(sc)
    by = {e[0]: r for e, r in zip(tr.CATALOGUE['big'], recs)}
    done = lit = 0
    for name in ('big_lds_15x40', 'big_one_wave_8x8'):       # a 229 x 32 and an 80 x 32 texture
        base, sh, sw = plans[by[name]['i']], by[name]['tex_h'], by[name]['tex_w']
        cases = []
        for tw in (1, 63, 64, 65):
            # a translation: pixel (x, y) reads the window at (s + x, ..), s = every offset at which a window crosses a side
            for s in (-4, -3, -2, -1, sw - 3, sw - 2, sw - 1, sw):
                cases.append((tw, 3, [1, 0, s + 1.25, 0, 1, sh // 2 + 0.4, 0, 0, 1]))
            for s in (-4, -3, -2, -1, sh - 3, sh - 2, sh - 1, sh):
                cases.append((tw, 5, [0.25, 0, sw // 2 + 0.3, 0, 1, s + 1.25, 0, 0, 1]))
            cases.append((tw, 4, [1, 0, 3.5, 0, 1, 7.5, 0, 1, -1]))             # W = 0 on row 1
            cases.append((tw, 4, [1, 0, 3.5, 0, 1, 7.5, 1, 0, -2]))             # W = 0 at column 2
            for a in (1e6, -1e6, 1e9, -1e9):                                     # coordinates that saturate at +-32768 and at +-2^31
                cases.append((tw, 3, [a, 0, 5.0, 0, 1, 9.0, 0, 0, 1]))
                cases.append((tw, 3, [1, 0, 5.0, 0, a, 9.0, 0, 0, 1]))
        cases.append((128, 64, [0.2, 0.01, -1.0, 0.02, 3.0, -2.0, 1e-4, 2e-4, 1]))   # blocks of 64 columns, a perspective
        for tw, th, mi in cases:
            rc, out, ref = _big(_hand_plan(base, tw, th, mi), db)
            assert rc == 0, (name, tw, th, mi, rc)
            done += 1
            lit += out.max() > 0
    assert done == 2 * (4 * 26 + 1) and lit > done // 2, (done, lit)
