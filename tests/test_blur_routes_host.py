"""CPU tier: the hand-built drop catalogue of tests/blur_routes.py reaches every defocus-blur route and both sides of each
threshold (according to the host classifier, which follows the compiled capacities), and the g++ build of the kernel
arithmetic renders the catalogue frames the way the numpy oracle does -- so the catalogue is on trial before the GPU sees it
(tests/test_gpu_blur_routes.py)."""
import numpy as np
import pytest

import blur_routes as br
import helpers as h


def _scene(tmp_path, entries, H=br.CAT_H, W=br.CAT_W):
    return h.Scene(tmp_path, H, W, 0, frames=[dict(id=0, t=2000, d=0, drops=br.catalogue_particles(entries, H, W))])


@pytest.fixture(scope='module')
def catalogue(tmp_path_factory):
    sc = _scene(tmp_path_factory.mktemp('cat'), br.CATALOGUE)
    drops = sc.product_drops(0)
    assert len(drops) == len(br.CATALOGUE)                  # nothing filtered: drop i is catalogue entry i
    return sc, drops, br.classify_drops(sc, drops)


def test_catalogue_entries_take_their_route(catalogue):
    """Every entry takes the route and carries the flags it was built for: a threshold that moves names the entry it moved."""
    _, _, recs = catalogue
    bad = []
    for (name, route, flags, *_), r in zip(br.CATALOGUE, recs):
        if r['route'] != route or r['flags'] != set(flags):
            bad.append((name, route, sorted(flags), '->', r['route'], sorted(r['flags']), dict(tw=r['tw'], th=r['th'], r1=r['r1'],
                        r2=r['r2'], ns=r['ns'], wo=r['wo'], ho=r['ho'])))
    assert not bad, bad


def test_catalogue_reaches_every_route(tmp_path, catalogue):
    _, _, recs = catalogue
    sc = _scene(tmp_path, br.BOUNDARY)
    brecs = br.classify_drops(sc, sc.product_drops(0))
    slow = h.Scene(tmp_path / 'slow', 240, 320, 0, frames=[dict(id=0, t=2000, d=0, drops=br.slow_cap_particles(300, 240, 320))])
    srecs = br.classify_drops(slow, slow.product_drops(0))
    table = {k: (a, b, c) for k, a, b, c in zip(br.ROUTES + br.FLAGS, *(br.census(x).values() for x in (recs, brecs, srecs)))}
    print('\n%-14s %9s %9s %9s' % ('route', 'catalogue', 'boundary', 'slow_cap'))
    for k, v in table.items():
        print('%-14s %9d %9d %9d' % ((k,) + v))
    lost = [k for k, v in table.items() if k != 'skipped' and sum(v) == 0]
    assert not lost, 'routes no catalogue frame reaches: %s' % lost
    assert table['beyond_cap'][2] > 0 and table['slow_radius'][2] + table['slow_halo'][2] > br.SLOW_CAP


def test_catalogue_thresholds(tmp_path, catalogue):
    """Both sides of each threshold, by entry: the values the routes are decided on."""
    _, _, recs = catalogue
    by = {e[0]: r for e, r in zip(br.CATALOGUE, recs)}
    # pad only / row radius 0: c in [0.1, 0.125) and [0.125, 0.25)
    assert (by['pad_only']['r1'], by['pad_only']['shift']) == (0, 1) and by['in_focus']['shift'] == 0
    assert (by['row_radius_0']['r1'], by['row_radius_0']['r2']) == (1, 0)
    # BS_X: tw * (php + 2 r1) = 512 is small, the next shape is not (the product is even: 513 cannot occur)
    for name, v in (('small_bs_x_512', 512), ('fused_bs_x_576', 576)):
        r = by[name]
        assert r['tw'] * (((r['eh'] + 3) & ~3) + 2 * r['r1']) == v, name
    # r1 = 31 / 32: both fused (with r2 = round(r1 / 2), BS_Y keeps k_blur_small below r1 ~ 12); 48 / 49: BR_MAX
    assert (by['r1_31']['r1'], by['r1_32']['r1'], by['r1_48']['r1'], by['r1_49']['r1']) == (31, 32, 48, 49)
    # ns = 8 / 9 / 17: one item per sub-tile, then items of two (the last one empty), of three
    assert [by[k]['ns'] for k in ('bands_8', 'bands_9', 'bands_17')] == [8, 9, 17]
    assert [n for _, n in by['bands_9']['items']] == [2, 2, 2, 2, 1, 0, 0, 0]
    assert [n for _, n in by['bands_17']['items']] == [3, 3, 3, 3, 3, 2, 0, 0]
    # slow drops wider than a unit's stride (BIG_GROUPS = 64 columns)
    assert by['slow_wide']['tw'] > 64 and by['halo_wide']['tw'] > 64
    # every border: some blurred footprint touches each edge of the frame
    boxes = [r['box'] for r in recs if r['live'] and r['r1'] > 0]
    assert min(b[0] for b in boxes) == 0 and min(b[1] for b in boxes) == 0
    assert max(b[2] for b in boxes) == br.CAT_W and max(b[3] for b in boxes) == br.CAT_H
    # RR_DROP_TOO_BIG: int(10 c) = 1024 is rendered (r1 next to MAX_R = 416), 1025 is skipped; an effective tile over 1024 rows
    sc = _scene(tmp_path, br.BOUNDARY)
    b = br.classify_drops(sc, sc.product_drops(0))
    assert (b[0]['shift'], b[0]['route'], b[1]['route']) == (1024, 'slow_radius', 'too_big')
    assert 400 < b[0]['r1'] <= 416 and b[0]['eh'] > 1024


def test_item_split_covers_every_subtile():
    for ns in range(1, 300):
        items = br.item_split(ns)
        assert len(items) == min(ns, br.ITEMS_PER_DROP)
        covered = [s for st0, n in items for s in range(st0, st0 + n)]
        assert covered == list(range(ns)), ns


def test_hostemu_matches_oracle_on_catalogue(catalogue):
    sc, drops, recs = catalogue
    bg, env = sc.frame_inputs(0)
    emu = h.emu_render(sc, bg, bg, env, drops)
    ref = h.oracle_render(sc, 0, bg, bg, env, faithful=False)
    br.check(emu, ref, recs, 'catalogue')
    assert emu['mask'].max() > 0


def test_hostemu_matches_oracle_past_slow_cap(tmp_path):
    sc = h.Scene(tmp_path, 240, 320, 0, frames=[dict(id=0, t=2000, d=0, drops=br.slow_cap_particles(300, 240, 320))])
    bg, env = sc.frame_inputs(0)
    drops = sc.product_drops(0)
    recs = br.classify_drops(sc, drops)
    emu = h.emu_render(sc, bg, bg, env, drops)
    ref = h.oracle_render(sc, 0, bg, bg, env, faithful=False)
    br.check(emu, ref, recs, 'slow_cap')
