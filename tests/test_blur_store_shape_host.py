"""CPU tier: the catalogue of tests/blur_store_shape.py reaches every class of the blur's column passes it was built for
(according to the host classifier), every blurred entry lies under its in-focus neighbour, and the g++ build of the kernel
arithmetic renders it the way the numpy oracle does -- the reference tests/test_gpu_blur_store_shape.py compares the GPU
with is pinned here, before the GPU sees the catalogue."""
import numpy as np
import pytest

import blur_routes as br
import blur_store_shape as ss
import helpers as h


@pytest.fixture(scope='module')
def frame(tmp_path_factory):
    sc = h.Scene(tmp_path_factory.mktemp('store_shape'), ss.H, ss.W, 0, frames=[dict(id=0, t=2000, d=0, drops=ss.particles())])
    drops = sc.product_drops(0)
    assert len(drops) == len(ss.entries())                  # nothing filtered: drop i is entry i
    return sc, drops, br.classify_drops(sc, drops)


def test_entries_take_their_route(frame):
    _, _, recs = frame
    bad = [(e[0], e[1], sorted(e[2]), '->', r['route'], sorted(r['flags'])) for e, r in zip(ss.entries(), recs)
           if r['route'] != e[1] or r['flags'] != set(e[2])]
    assert not bad, bad


def test_catalogue_reaches_every_class(frame):
    _, _, recs = frame
    reached = ss.classes(recs)
    print('\n' + '\n'.join('%-30s %s' % (k, reached.get(k)) for k in ss.REQUIRED))
    assert not [k for k in ss.REQUIRED if not reached.get(k)]
    # the four widths of each kernel's four-column branch are consecutive raw widths at one circle of confusion
    by = {e[0]: r for e, r in zip(ss.entries(), recs)}
    for names in (('small_w9', 'small_w10', 'small_w11', 'small_w12'), ('single_w20', 'single_w21', 'single_w22', 'single_w23')):
        rs = [by[n] for n in names]
        assert [r['tw'] - rs[0]['tw'] for r in rs] == [0, 1, 2, 3] and len({(r['r1'], r['r2']) for r in rs}) == 1
        assert [r['ew'] for r in rs] == [r['tw'] + 2 * r['r2'] for r in rs]


def test_neighbours_lie_over_their_blurred_tile(frame):
    """Drop 2k is blurred, drop 2k + 1 in focus, live, next in table order, its footprint inside the blurred one."""
    _, _, recs = frame
    for k in range(0, len(recs), 2):
        b, n = recs[k], recs[k + 1]
        assert b['live'] and b['r1'] > 0 and n['live'] and n['route'] == 'no_blur', (k, b['route'], n['route'])
        bx0, by0, bx1, by1 = b['box']
        nx0, ny0, nx1, ny1 = n['box']
        assert nx0 < nx1 and ny0 < ny1 and bx0 <= nx0 and nx1 <= bx1 and by0 <= ny0 and ny1 <= by1, (k, b['box'], n['box'])


def test_hostemu_matches_oracle(frame):
    sc, drops, recs = frame
    bg, env = sc.frame_inputs(0)
    emu = h.emu_render(sc, bg, bg, env, drops)
    ref = h.oracle_render(sc, 0, bg, bg, env, faithful=False)
    br.check(emu, ref, recs, 'store-shape catalogue')
    assert emu['mask'].max() > 0
