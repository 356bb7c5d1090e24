"""GPU tier: RR_OPT_STREAK_LEAN on the device (k_plan hands the mode to plan_drop) -- rr_render_frames on the catalogue of
tests/streak_lean_cases.py against the frozen oracle, by composition: mask bit-exact, image within 1 LSB, statuses equal, under both
compositors (RR_OPT_COMPOSITE_F64 0 / 1) and with and without tile sharing (RR_OPT_DEDUP 0 / 1: the same bits); every entry alone in a
batch of single-drop frames; option 0 on the same records gives what the library gave before the option was touched."""
import numpy as np
import pytest

import helpers as h
import streak_lean_cases as slc

pytestmark = pytest.mark.gpu

KEYS = ('status', 'mask', 'mask_i32', 'image_u8')


@pytest.fixture(scope='module')
def setup(built, tmp_path_factory):
    sc = h.Scene(tmp_path_factory.mktemp('lean_scene'), slc.H, slc.W, 10)
    bg, env = sc.frame_inputs(0)
    recs = slc.records(tmp_path_factory.mktemp('lean_records'))
    return sc, bg, env, recs


def _rh(sc):
    rh = h.hb.RainHip(0)
    rh.set_streak_db(sc.db.streaks_light)
    rh.set_camera(sc.cam)
    return rh


def _frame(sc, bg, env, drops):
    return dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=drops)


@pytest.mark.parametrize("f64", [0, 1])
def test_catalogue_against_the_oracle_composition(setup, f64):
    sc, bg, env, recs = setup
    ref = slc.oracle_lean(sc, bg, env, recs)
    plain_ref = h.emu_render(sc, bg, bg, env, recs)                # the host build of the reference's rule
    rh = _rh(sc)
    try:
        rh.set_option(h.hb.RR_OPT_COMPOSITE_F64, f64)
        before = rh.render_frames([_frame(sc, bg, env, recs)])[0]          # the option not yet touched
        outs = {}
        for dedup in (1, 0):
            rh.set_option(h.hb.RR_OPT_DEDUP, dedup)
            rh.set_option(h.hb.RR_OPT_STREAK_LEAN, 1)
            # the catalogue twice in one batch: with tile sharing on, the second frame's tiles are the first one's
            two = rh.render_frames([_frame(sc, bg, env, recs), _frame(sc, bg, env, recs)])
            for k, out in enumerate(two):
                slc.check(out, ref, 'catalogue, f64 %d, dedup %d, frame %d' % (f64, dedup, k))
            outs[dedup] = two[0]
            rh.set_option(h.hb.RR_OPT_STREAK_LEAN, 0)
            off = rh.render_frames([_frame(sc, bg, env, recs)])[0]
            for key in KEYS:
                assert np.array_equal(off[key], before[key]), (key, dedup)
        for key in KEYS:
            assert np.array_equal(outs[0][key], outs[1][key]), key         # both dedup settings: the same bits
        slc.check(before, plain_ref, 'option 0')
        assert not np.array_equal(before['mask'], outs[1]['mask'])
    finally:
        rh.close()


def test_every_entry_alone_and_the_overlap_in_both_orders(setup):
    """One batch: a frame per catalogue entry, and the two overlapping drops of opposite lean in both table orders."""
    sc, bg, env, recs = setup
    tables = [recs[i:i + 1] for i in range(len(recs))]
    a, b = slc.NAMES.index('overlap_a'), slc.NAMES.index('overlap_b')
    tables += [recs[[a, b]], recs[[b, a]]]
    names = slc.NAMES + ['overlap a, b', 'overlap b, a']
    rh = _rh(sc)
    try:
        rh.set_option(h.hb.RR_OPT_STREAK_LEAN, 1)
        outs = rh.render_frames([_frame(sc, bg, env, t) for t in tables])
    finally:
        rh.close()
    for name, t, out in zip(names, tables, outs):
        ref = slc.oracle_lean(sc, bg, env, t)
        slc.check(out, ref, name)
        assert np.all(ref['status'] == 0) and (ref['mask'] > 0).any(), name
