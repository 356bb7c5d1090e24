"""CPU tier: the catalogue of tests/blur_small_pipeline.py does what it was built for, by the host classifier and the launch's
grid formula: every drop takes the small route, the three tables have the lengths that give waves of 0, 1, 2, 3 and 4
iterations (and workgroups whose waves differ), every branch of the row pass and of the column pass is taken in a second or
later iteration, and some wave takes, one after the other, drops of different radius and different branches.  The g++ build of
the kernel arithmetic renders table B the way the numpy oracle does (tests/test_gpu_blur_small_pipeline.py compares the GPU
with that build)."""
import pytest

import blur_routes as br
import blur_small_pipeline as sp
import helpers as h


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    sc = h.Scene(tmp_path_factory.mktemp('small_pipeline'), sp.H, sp.W, 0, frames=sp.frames())
    drops = [sc.product_drops(t) for t in range(3)]
    assert [len(d) for d in drops] == list(sp.N_TABLE)          # nothing filtered: drop i is entry i
    return sc, drops, [br.classify_drops(sc, d) for d in drops]


def test_every_drop_takes_the_small_route(tables):
    _, _, recs = tables
    for t in range(3):
        bad = [(e[0], r['route'], sorted(r['flags'])) for e, r in zip(sp.entries(t), recs[t])
               if r['route'] != 'small' or not r['live'] or r['flags'] != set(e[2])]
        assert not bad, bad[:8]
        assert br.expected_counts(recs[t])[2] == sp.N_TABLE[t]


def test_grid_is_capped_at_64_workgroups():
    assert sp.grid_x(max(sp.N_TABLE), sp.N_FRAMES) == 64
    assert sp.grid_x(max(sp.N_TABLE), 1) > 64                  # a single frame of table A: one drop per wave


def test_census_has_no_empty_class(tables):
    _, _, recs = tables
    found = sp.census(recs)
    print('\n' + '\n'.join('%-28s %5d  e.g. %s' % (k, len(found[k]), found[k][:2]) for k in sp.REQUIRED))
    assert not [k for k in sp.REQUIRED if not found[k]]
    assert not found['neighbours_same_r1'], found['neighbours_same_r1'][:8]
    # ... in every table with a second iteration, table B's three second drops among them
    for t, n in ((0, 2 * 256 + 5), (1, 3)):
        assert len([v for v in found['neighbours_differ'] if v[0] == t]) > 0 and \
            len([v for k in sp.ROW_CLASSES for v in found[k + '_later'] if v[0] == t]) == n, t
    # table A: waves 0 .. 4 four iterations, the others three; B: 0 .. 2 two, the others one; C: 0 .. 4 one, the others none
    for t, (first, n_hi, n_lo) in enumerate(((5, 4, 3), (3, 2, 1), (5, 1, 0))):
        trips = {}
        for b, w, j, _ in sp.schedule(recs[t], max(sp.N_TABLE), sp.N_FRAMES)[1]:
            trips[4 * b + w] = max(trips.get(4 * b + w, 0), j + 1)
        assert [trips.get(v, 0) for v in range(256)] == [n_hi] * first + [n_lo] * (256 - first), t


def test_single_frame_takes_one_drop_per_wave(tables):
    """Why the one-frame catalogues cannot stand in: alone, even table A gives no wave a second drop."""
    _, _, recs = tables
    assert all(j == 0 for _, _, j, _ in sp.schedule(recs[0], sp.N_TABLE[0], 1)[1])


def test_hostemu_matches_oracle(tables):
    sc, drops, recs = tables
    bg, env = sc.frame_inputs(1)
    emu = h.emu_render(sc, bg, bg, env, drops[1])
    ref = h.oracle_render(sc, 1, bg, bg, env, faithful=False)
    br.check(emu, ref, recs[1], 'small-pipeline table B')
    assert emu['mask'].max() > 0
