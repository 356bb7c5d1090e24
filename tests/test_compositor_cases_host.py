"""CPU tier: the compositor catalogues of tests/compositor_cases.py on trial before the GPU sees them
(tests/test_gpu_compositor_cases.py).  Every class is reached according to the host classifier; the g++ build of the kernel
arithmetic renders every catalogue frame the way the numpy oracle does; and every stack and overlap group is sensitive to the
order of its drops -- conditions on the inputs, checked on the oracle and never on the code under test."""
import time

import numpy as np
import pytest

import compositor_cases as cc

TIMES = {}


def _timed(key, fn):
    t = time.time()
    out = fn()
    TIMES[key] = TIMES.get(key, 0.0) + time.time() - t
    return out


@pytest.fixture(scope='module')
def cat(tmp_path_factory):
    """name -> Case, with the host build's rendering (case.ref_emu) and the classifier's lists (case.listed, case.boxes)."""
    tpl = cc.Templates(tmp_path_factory.mktemp('tpl'))
    cases = [cc.seams(tmp_path_factory.mktemp('sl'), tpl, 'low'), cc.seams(tmp_path_factory.mktemp('sh'), tpl, 'high'),
             cc.lengths(tmp_path_factory.mktemp('le'), tpl), cc.indices(tmp_path_factory.mktemp('in'), tpl),
             cc.segment(tmp_path_factory.mktemp('sg'), tpl)] + cc.shapes(lambda n: tmp_path_factory.mktemp(n), tpl)
    out = {}
    for c in cases:
        c.ref_emu = _timed('host build, ' + c.name, c.emu)
        c.listed, c.boxes = cc.listed_drops(c.scene, c.drops, c.ref_emu['status'])
        out[c.name] = c
    return out


@pytest.fixture(scope='module')
def oracle_refs(cat):
    """The oracle's rendering of seams, lengths and shapes (whole tables) and of the rendering records of indices."""
    out = {}
    for name, c in cat.items():
        if name == 'segment':
            continue
        drops = c.drops if name != 'indices' else c.drops[np.setdiff1d(np.arange(len(c.drops)), c.filler)]
        out[name] = _timed('oracle, ' + name, lambda: c.oracle(drops))
    return out


def _entry_index(c):
    return {i: e for e in c.entries for i in e['idx']}


def _quadrants_reached(box, geom):
    out = set()
    for tyi in range(box[1] // geom['th'], (box[3] - 1) // geom['th'] + 1):
        for txi in range(box[0] // geom['tw'], (box[2] - 1) // geom['tw'] + 1):
            for q in range(4):
                qx0, qy0 = txi * geom['tw'] + (q & 1) * geom['sx'], tyi * geom['th'] + (q >> 1) * geom['sy']
                qx1 = (txi + 1) * geom['tw'] if q & 1 else qx0 + geom['sx']
                qy1 = (tyi + 1) * geom['th'] if q >> 1 else qy0 + geom['sy']
                if cc._reaches(box, qx0, qy0, qx1, qy1):
                    out.add(((tyi, txi), q))
    return out


def _census(cat):
    """{catalogue: {class: count}}: what the classifier finds, not what the builders meant."""
    out = {}
    for name in ('seams_low', 'seams_high'):
        c, n = cat[name], {}
        for geom in cc.GEOMS:
            for k in cc.SEAM_CLASSES:
                n['%s %s' % (geom['name'], k)] = 0
            for i in c.listed:
                for k in cc.seam_relations(c.boxes[i], geom):
                    n['%s %s' % (geom['name'], k)] += 1
            n[geom['name'] + ' four_quadrants'] = sum(any(len({q for t2, q in _quadrants_reached(c.boxes[i], geom) if t2 == t}) == 4
                                                      for t, _ in _quadrants_reached(c.boxes[i], geom)) for i in c.listed)
            n[geom['name'] + ' four_tiles'] = sum(len({t for t, _ in _quadrants_reached(c.boxes[i], geom)}) >= 4 for i in c.listed)
            # only the last row of a lane's first pixels and the first row of its second pixels
            n[geom['name'] + ' rows_7_8'] = sum(c.boxes[i][1] % geom['sy'] == 7 and c.boxes[i][3] - c.boxes[i][1] == 2 for i in c.listed)
        n['four_coarse'] = sum(len({(y // cc.CTILE, x // cc.CTILE) for x in (c.boxes[i][0], c.boxes[i][2] - 1) for y in (c.boxes[i][1], c.boxes[i][3] - 1)}) == 4
                               for i in c.listed)
        raw = {i: e['raw_box'] for e in c.entries for i in e['idx']}
        n['crop_left'] = sum(raw[i][0] < 0 == c.boxes[i][0] for i in c.listed)
        n['crop_top'] = sum(raw[i][1] < 0 == c.boxes[i][1] for i in c.listed)
        n['crop_right'] = sum(raw[i][2] > c.W == c.boxes[i][2] for i in c.listed)
        n['crop_bottom'] = sum(raw[i][3] > c.H == c.boxes[i][3] for i in c.listed)
        n['record starts at x < 0'] = sum(int(c.drops['x0'][i]) < 0 for i in c.listed)
        n['record starts at y < 0'] = sum(int(c.drops['y0'][i]) < 0 for i in c.listed)
        n['last 16x32 row'] = sum(c.boxes[i][3] > (c.H - 1) // 32 * 32 for i in c.listed)
        for label, names in (('blurred (effective tile)', ('blur', 'blur2')), ('pad only', ('padonly',)), ('Big', ('big', 'big2')), ('oblique', ('o9', 'o5'))):
            n[label] = sum(e.get('tpl') in names for e in c.entries)
        n['overlap groups'] = len(c.groups())
        out[name] = n
    c, n = cat['lengths'], {}
    for geom in cc.GEOMS:
        wl = cc.work_lists(c.H, c.W, c.listed, c.boxes, geom)
        totals = [len(q) for ps in wl['pieces'].values() for quads in ps for q in quads]
        for v in cc.TOTALS:
            n['%s total %d' % (geom['name'], v)] = totals.count(v)
        for v in cc.COARSE_NS:
            n['n %d' % v] = [len(v2) for v2 in wl['coarse'].values()].count(v)
        hit255 = hit256 = gap = 0
        for (tyi, txi), ps in wl['pieces'].items():
            lst = wl['coarse'][(tyi * geom['th'] // cc.CTILE, txi * geom['tw'] // cc.CTILE)]
            for q in range(4):
                tot = [len(quads[q]) for quads in ps]
                hit255 += len(lst) > 255 and lst[255] in ps[0][q]
                hit256 += len(lst) > 256 and lst[256] in ps[1][q]
                gap += any(tot[k] == 0 and any(tot[:k]) and any(tot[k + 1:]) for k in range(len(tot)))
        n[geom['name'] + ' hit at list position 255'] = hit255
        n[geom['name'] + ' hit at list position 256'] = hit256
        n[geom['name'] + ' empty piece between two'] = gap
        alt = 0
        for lst in wl['coarse'].values():
            tiles = [(c.boxes[i][1] // geom['th'], c.boxes[i][0] // geom['tw']) for i in lst]
            alt = max(alt, sum(a != b for a, b in zip(tiles, tiles[1:])))
        n[geom['name'] + ' tile changes along one list'] = alt
    K = c.ref_emu['K']
    n['stacks'] = len(c.groups())
    n['stacks of >= 6 with six colour constants'] = sum(len({tuple(np.round(K[i], 6)) for i in idx}) >= 6 for idx in c.groups().values() if len(idx) >= 6)
    n['stacks of >= 6'] = sum(len(idx) >= 6 for idx in c.groups().values())
    out['lengths'] = n
    c, n = cat['indices'], {}
    n['records'] = len(c.drops)
    n['listed'] = len(c.listed)
    n['filler: status 0, empty box'] = sum(c.ref_emu['status'][i] == 0 and not (c.boxes[i][0] < c.boxes[i][2] and c.boxes[i][1] < c.boxes[i][3]) for i in c.filler)
    for i in cc.SPECIAL_INDICES:
        n['index %d listed' % i] = int(i in c.listed)
    ent = _entry_index(c)
    for a, b in ((cc.BIN_SEG - 1, cc.BIN_SEG), (32767, 32768)):
        n['%d and %d in one quadrant' % (a, b)] = int(a in ent and b in ent and ent[a] is ent[b])
    out['indices'] = n
    c, n = cat['segment'], {}
    n['records'] = len(c.drops)
    n['listed'] = len(c.listed)
    n['quadrants with drops of both segments'] = sum(min(e['idx']) < cc.BIN_SEG <= max(e['idx']) for e in c.entries)
    out['segment'] = n
    n = {}
    for name, W, H in cc.SHAPES:
        n['%s: 16x32 tiles' % name] = cc.tile_count(H, W, cc.GEOM32)
        n['%s: 16x16 tiles' % name] = cc.tile_count(H, W, cc.GEOM64)
        n['%s: listed' % name] = len(cat[name].listed)
    c = cat['wide']
    n['wide: coarse tiles per row'] = -(-c.W // cc.CTILE)
    wl = cc.work_lists(c.H, c.W, c.listed, c.boxes, cc.GEOM32)
    n['wide: n of coarse tile 63'] = len(wl['coarse'][(0, 63)])
    n['wide: n of coarse tile 64'] = len(wl['coarse'][(0, 64)])
    n['wide: boxes across x = 4096'] = sum(c.boxes[i][0] < 4096 < c.boxes[i][2] for i in c.listed)
    out['shapes'] = n
    return out


def test_catalogue_reaches_every_class(cat):
    """The census, and: no class empty, every total / n / index the catalogues were built for occurs, every box where its entry says."""
    cen = _census(cat)
    for name, n in cen.items():
        print('\n%s' % name)
        for k, v in n.items():
            print('  %-46s %6d' % (k, v))
    for name, n in cen.items():
        empty = [k for k, v in n.items() if v == 0]
        assert not empty, '%s: classes no entry reaches: %s' % (name, empty)
    for c in cat.values():
        bad = [(e['name'], e['boxes'][k], c.boxes[i]) for e in c.entries for k, i in enumerate(e['idx']) if tuple(c.boxes[i]) != tuple(e['boxes'][k])]
        assert not bad, '%s: boxes not where the entry says: %s' % (c.name, bad[:8])
        want = sorted(i for e in c.entries for i, b in zip(e['idx'], e['boxes']) if b[0] < b[2] and b[1] < b[3])
        assert c.listed == want, '%s: listed drops' % c.name
    n = cen['indices']
    assert n['records'] == 65536 and 50 <= n['listed'] <= 70 and n['filler: status 0, empty box'] == 65536 - n['listed']
    assert cen['segment']['records'] == cen['segment']['listed'] == cc.BIN_SEG + 40
    assert [cen['shapes']['%s: 16x32 tiles' % s[0]] for s in cc.SHAPES] == [1, 3, 7, 8, 9]       # fewer than, as many as, more than the shares
    assert cc.XCD_SHARES == 8
    assert cen['shapes']['wide: coarse tiles per row'] == 65 > cc.BIN_ROWS_MAX_CT
    assert cen['lengths']['stacks of >= 6 with six colour constants'] == cen['lengths']['stacks of >= 6']
    # the lower waves of the last 16 x 32 tile row own no pixel in one variant and some in the other
    assert 0 < cc.SEAMS_H['low'] % 32 <= 16 < cc.SEAMS_H['high'] % 32 and cc.SEAMS_W % 16
    # k_composite32's batches and tails: totals of one, two and three batches, tails of 0, 1 and 2 entries behind the triples
    pcs = [cc.piece_classes(v) for v in cc.TOTALS]
    assert {p['batches'] for p in pcs} == {1, 2, 3} and {p['tail'] for p in pcs} == {0, 1, 2}


def test_seam_entries_show_on_both_sides(cat):
    """An entry that overlaps a seam by one pixel has alpha > 0 on that pixel row / column (host build, the entry alone): a list
    that misses it there changes the mask."""
    for name in ('seams_low', 'seams_high'):
        c = cat[name]
        for e in c.entries:
            rel = e['name'].split('_', 1)[-1]
            if e['name'][0] not in 'xy' or rel not in ('over_lo', 'over_hi'):
                continue
            m = c.emu(c.drops[e['idx']])['mask']
            x0, y0, x1, y1 = e['box']
            strip = {('x', 'over_lo'): m[y0:y1, x1 - 1], ('x', 'over_hi'): m[y0:y1, x0], ('y', 'over_lo'): m[y1 - 1, x0:x1], ('y', 'over_hi'): m[y0, x0:x1]}
            assert (strip[(e['name'][0], rel)] > 0).any(), e['name']


def test_hostemu_matches_oracle_on_catalogues(cat, oracle_refs):
    for name, ref in oracle_refs.items():
        c = cat[name]
        if name == 'indices':
            # the oracle takes ~6 ms per record, off-frame ones too: it renders the rendering records alone
            keep = np.setdiff1d(np.arange(len(c.drops)), c.filler)
            emu = dict(c.ref_emu, status=c.ref_emu['status'][keep])
            assert not c.ref_emu['status'][c.filler].any()
        else:
            emu = c.ref_emu
        cc.check(emu, ref, c, 'host build vs oracle')
        assert not ref['status'].any() and ref['mask'].max() > 0
    print('\nseconds: %s' % {k: round(v, 2) for k, v in TIMES.items()})


def test_hostemu_matches_oracle_across_bin_seg(cat):
    """The BIN_SEG + 40 table is the host build's to judge on the GPU (the oracle would take a minute): here both render the
    records around the segment boundary."""
    c = cat['segment']
    window = c.drops[cc.BIN_SEG - 300:cc.BIN_SEG + 40]
    cc.check(c.emu(window), c.oracle(window), c, 'segment window')


def _margins(c, fwd, rev, before_last, groups):
    """{group: (entries, pixels of its box whose mask bits differ under reversal, largest image_u8 difference there, range of the
    covered composite before the last entry)}."""
    out = {}
    for g, idx in groups.items():
        x0, y0, x1, y1 = c.group_box(g)
        f, r, b = fwd[g], rev[g], before_last[g]
        cov = b['mask'][y0:y1, x0:x1] > 0
        v = b['rainy_bg'][y0:y1, x0:x1][cov]
        out[g] = (len(idx), int((f['mask'][y0:y1, x0:x1] != r['mask'][y0:y1, x0:x1]).sum()),
                  int(np.abs(f['image_u8'][y0:y1, x0:x1].astype(int) - r['image_u8'][y0:y1, x0:x1].astype(int)).max()),
                  float(v.min()) if v.size else 0.5, float(v.max()) if v.size else 0.5)
    return out


def _assert_sensitive(name, margins):
    print('\n%s: group, entries, mask pixels that differ under reversal, image LSB, composite range before the last entry' % name)
    for g, m in margins.items():
        print('  %-14s %4d %4d %3d  %.3f .. %.3f' % ((g,) + m))
    print('  minimum image difference of a group: %d LSB' % min(m[2] for m in margins.values() if m[0] >= 2))
    for g, (n, mask_px, lsb, lo, hi) in margins.items():
        # A list of one entry has no order.  The mask of two is a + b in either order, the same bits; the image still tells.
        if n >= 3:
            assert mask_px >= 1, '%s %s: the reversed stack has the same mask' % (name, g)
        if n >= 2:
            assert lsb >= 3, '%s %s: the reversed stack is within %d LSB' % (name, g, lsb)
        assert 0.0 < lo and hi < 1.0, '%s %s: the composite saturates before the last entry (%r .. %r)' % (name, g, lo, hi)


@pytest.mark.parametrize('name', ['seams_low', 'seams_high'])
def test_overlap_groups_are_order_sensitive(cat, name):
    """Each overlap group alone through the oracle, forwards, reversed and without its last entry."""
    c = cat[name]
    groups = c.groups()
    fwd = {g: c.oracle(c.drops[idx]) for g, idx in groups.items()}
    rev = {g: c.oracle(c.drops[idx[::-1]]) for g, idx in groups.items()}
    last = {g: c.oracle(c.drops[idx[:-1]]) for g, idx in groups.items()}
    _assert_sensitive(name, _margins(c, fwd, rev, last, groups))
    emu = c.ref_emu
    assert all(emu['status'][i] == 0 for e in c.entries for i in e['idx']) and sorted(c.listed) == list(range(len(c.drops)))


def test_stacks_are_order_sensitive(cat, oracle_refs):
    """The stacks of `lengths` share no pixel, so the whole table reversed reverses every stack, and the table without each
    stack's last entry stops every stack one short."""
    c = cat['lengths']
    groups = c.groups()
    boxes = [c.group_box(g) for g in groups]
    assert not any(cc._reaches(a, *b) for k, a in enumerate(boxes) for b in boxes[k + 1:])
    rev = _timed('oracle, lengths reversed', lambda: c.oracle(c.drops[::-1]))
    lasts = {idx[-1] for idx in groups.values()}
    short = _timed('oracle, lengths before the last entries', lambda: c.oracle(c.drops[[i for i in range(len(c.drops)) if i not in lasts]]))
    m = _margins(c, {g: oracle_refs['lengths'] for g in groups}, {g: rev for g in groups}, {g: short for g in groups}, groups)
    _assert_sensitive('lengths', m)
    assert sorted(c.listed) == list(range(len(c.drops)))
    print('\nseconds: %s' % {k: round(v, 2) for k, v in TIMES.items()})


def test_localisation_names_tile_quadrant_and_lane_pixel(cat):
    """check() on a rendering with one wrong pixel names the entry, the tile, the quadrant and the lane's pixel."""
    c = cat['seams_low']
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.ref_emu.items()}
    bad['mask'][48 + 9, 24] += 1.0                        # 16 x 32: tile row 1, column 1, lower right quadrant, row 9 of it
    with pytest.raises(AssertionError) as err:
        cc.check(bad, c.ref_emu, c, 'planted', cc.GEOM32)
    msg = str(err.value)
    assert "((1, 1), 3, 'second')" in msg and 'quad32' in msg and 'seams_low' in msg, msg
    assert cc.locate(24, 57, cc.GEOM64) == ((3, 1), 3, 'first') and cc.locate(23, 47, cc.GEOM32) == ((1, 1), 0, 'second')
