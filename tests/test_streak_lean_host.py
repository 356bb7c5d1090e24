"""CPU tier: RR_OPT_STREAK_LEAN (rr_device.h plan_drop, lean = 1) -- a rotated tile's flip (x1 > x0) and corner (min x, min y) from
the streak's own end points.

  6. the g++ build of the renderer with the mode on (tests/hostemu/lean_emu.cpp: hostemu.cpp through plan_drop's defaulted argument)
     against the frozen oracle, by composition (streak_lean_cases.oracle_lean), on the catalogue of hand-made streaks: mask float64 and
     int32 bit-exact, image within 1 LSB, statuses equal; with the mode off the same build is libhostemu.so and the oracle as it is;
  7. where the two rules agree the DropPlan is identical; where they do not, only flip and placement move;
     what the rule and the composition rest on: which of the oracle's two tiles leans like its streak, in all four directions."""
import numpy as np
import pytest

import helpers as h
import streak_lean_cases as slc
from oracle import render as orc


@pytest.fixture(scope='module')
def setup(built, tmp_path_factory):
    sc = h.Scene(tmp_path_factory.mktemp('lean_scene'), slc.H, slc.W, 10)
    bg, env = sc.frame_inputs(0)
    recs = slc.records(tmp_path_factory.mktemp('lean_records'))
    return sc, bg, env, recs


def _idx(*names):
    return [slc.NAMES.index(n) for n in names]


# ---- 6. the host build == the oracle composition -------------------------------------------------------------------
def test_catalogue_against_the_oracle_composition(setup):
    sc, bg, env, recs = setup
    out = slc.emu_render(sc, bg, env, recs, 1)
    ref = slc.oracle_lean(sc, bg, env, recs)
    slc.check(out, ref, 'catalogue')
    assert np.all(ref['status'] == 0) and (ref['mask'] > 0).sum() > 300
    # the mode does something: the reference's rule gives another frame
    plain = slc.emu_render(sc, bg, env, recs, 0)
    assert not np.array_equal(plain['mask'], out['mask'])


@pytest.mark.parametrize("name", slc.NAMES)
def test_every_entry_alone(setup, name):
    """One drop per frame: a wrong tile cannot hide under a neighbour."""
    sc, bg, env, recs = setup
    one = recs[_idx(name)]
    out = slc.emu_render(sc, bg, env, one, 1)
    ref = slc.oracle_lean(sc, bg, env, one)
    slc.check(out, ref, name)
    assert ref['status'][0] == 0 and (ref['mask'] > 0).any(), name


def test_overlapping_drops_of_opposite_lean_in_both_orders(setup):
    sc, bg, env, recs = setup
    for order in (_idx('overlap_a', 'overlap_b'), _idx('overlap_b', 'overlap_a')):
        two = recs[order]
        out = slc.emu_render(sc, bg, env, two, 1)
        slc.check(out, slc.oracle_lean(sc, bg, env, two), 'overlap %s' % order)
        a, b = (slc.emu_render(sc, bg, env, two[k:k + 1], 1)['mask'] > 0 for k in (0, 1))
        assert (a & b).sum() > 0                                  # they do share pixels
        assert not np.array_equal(a, b)


def test_mode_off_is_the_unchanged_build_and_the_unchanged_oracle(setup):
    sc, bg, env, recs = setup
    off = slc.emu_render(sc, bg, env, recs, 0)
    base = h.emu_render(sc, bg, bg, env, recs)                    # libhostemu.so
    for k in ('status', 'mask', 'mask_i32', 'image_u8', 'rainy_bg'):
        assert np.array_equal(off[k], base[k]), k
    textures, _ = sc.oracle_db()
    ref = orc.render_drop_records(bg, bg, env, sc.omega, recs, textures, sc.ocam)
    slc.check(off, ref, 'mode off')


# ---- 7. the plans ------------------------------------------------------------------------------------------------------
PLACEMENT = ('flip', 'vis_x0', 'vis_y0', 'vis_w', 'vis_h', 'crop_x', 'crop_y')


def test_plans_where_the_rules_agree_and_where_they_do_not(setup):
    sc, _, _, recs = setup
    p0, s0 = slc.emu_plan(sc, recs, 0)
    p1, s1 = slc.emu_plan(sc, recs, 1)
    base, sb = h.emu_plan(sc, recs)
    assert p0.tobytes() == base.tobytes() and np.array_equal(s0, sb)
    same = _idx('right_down_right_half', 'big', 'big_left_down')
    for i in same:                                               # ends in the right half, or Big: an identical DropPlan
        assert p0[i:i + 1].tobytes() == p1[i:i + 1].tobytes(), slc.NAMES[i]
    assert int(p1[same[0]]['flip']) == 1
    moved = 0
    for i, (r, name) in enumerate(zip(recs, slc.NAMES)):
        a, b = p0[i], p1[i]
        if int(r['type']) == 0:
            assert a.tobytes() == b.tobytes(), name
            continue
        assert int(b['flip']) == int(slc.wanted_flip(r)), name
        assert int(a['flip']) == int(int(r['x1']) > slc.W // 2), name
        for f in h.PLAN_DTYPE.names:                              # nothing else moves: size, rotation, resize route, blur, blend scalars
            if f not in PLACEMENT:
                assert a[f].tobytes() == b[f].tobytes(), (name, f)
        # the corner: the tile is placed from (min x, min y) - shift, clamped to the frame
        shift = int(b['shift'])
        cx, cy = min(int(r['x0']), int(r['x1'])) - shift, min(int(r['y0']), int(r['y1'])) - shift
        assert (int(b['vis_x0']), int(b['vis_y0'])) == (min(max(cx, 0), slc.W), min(max(cy, 0), slc.H)), name
        assert (int(b['crop_x']), int(b['crop_y'])) == (max(-cx, 0) if cx < 0 else 0, max(-cy, 0) if cy < 0 else 0), name
        moved += a.tobytes() != b.tobytes()
    assert moved >= 8


LEANING = ('right_down_left_half', 'left_down_right_half', 'right_up', 'left_up', 'right_down_right_half', 'small_right_down',
           'small_left_down', 'corner_left_of_frame', 'corner_above_frame', 'starts_outside_left', 'starts_outside_right', 'overlap_a',
           'overlap_b', 'blurred_left_down', 'blurred_small_right_up')


def test_the_rule_makes_the_tile_lean_like_its_streak(setup):
    """What the rule and the composition rest on, measured on the oracle's own tiles.  The rotation is by -acos((y1 - y0) / n), so a
    streak that runs UP the image gets a tile turned by more than 90 degrees: with the flip taken the tile's mass has the x-y
    covariance sign(y1 - y0), without it the opposite.  The streak's own is sign((x1 - x0) (y1 - y0)): the two agree exactly when the
    flip is taken for x1 > x0 -- in all four directions.  (Taking it for (x1 - x0) (y1 - y0) > 0 mirrors the two upward ones.)
    The oracle's corner is the start point, whichever flip; the tile's size does not depend on it."""
    sc, _, _, recs = setup
    textures, _ = sc.oracle_db()
    for name in LEANING:
        r = recs[slc.NAMES.index(name)]
        dx, dy = int(r['x1']) - int(r['x0']), int(r['y1']) - int(r['y0'])
        for fake, flipped in ((slc.ALWAYS_FLIP, True), (slc.NEVER_FLIP, False)):
            drop = orc.Streak()
            drop.image_position_start = np.array([int(r['x0']), int(r['y0'])])
            drop.image_position_end = np.array([int(r['x1']), int(r['y1'])])
            drop.max_width, drop.length, drop.drop_type = int(r['max_width']), int(r['length']), orc.DropType(int(r['type']))
            tile, minC = orc.make_drop_tile(drop, textures[int(r['tex_index'])], 0.0, fake, slc.H, rot=(float(r['rot_cos']), float(r['rot_sin'])))
            cov = slc.tile_covariance(tile[..., 3])
            assert abs(cov) > 0.5 and np.sign(cov) == (np.sign(dy) if flipped else -np.sign(dy)), (name, flipped, cov)
            if flipped == slc.wanted_flip(r):
                assert np.sign(cov) == np.sign(dx * dy), (name, cov)          # the rule's tile leans like the streak
            assert tuple(minC) == (int(r['x0']), int(r['y0']))
            assert tile.shape[:2] == (max(abs(dy), 2), max(abs(dx), int(r['max_width']) + 2))
    assert {(np.sign(int(recs[slc.NAMES.index(n)]['x1']) - int(recs[slc.NAMES.index(n)]['x0'])),
             np.sign(int(recs[slc.NAMES.index(n)]['y1']) - int(recs[slc.NAMES.index(n)]['y0']))) for n in LEANING} == {(1, 1), (-1, 1), (1, -1), (-1, -1)}


def test_the_rendered_mask_leans_like_the_streak(setup):
    """End to end on the host build with the mode on: the mask of every leaning entry alone has the covariance sign of its streak."""
    sc, bg, env, recs = setup
    for name in LEANING:
        if name.startswith('corner') or name.startswith('starts_outside'):
            continue                                              # (cropped by the frame: the visible part is too short to tell)
        r = recs[slc.NAMES.index(name)]
        m = slc.emu_render(sc, bg, env, recs[_idx(name)], 1)['mask']
        want = np.sign((int(r['x1']) - int(r['x0'])) * (int(r['y1']) - int(r['y0'])))
        assert np.sign(slc.tile_covariance(m)) == want, name
