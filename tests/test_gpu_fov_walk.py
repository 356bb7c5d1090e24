"""GPU tier: k_fov_dda's walk by chained records (rr_device.h fov_walk_make_records + FovWalk; tests/test_fov_walk_host.py
pins it on the CPU) on the polygons the benchmark's first frame never shows it: test_gpu_fov_order's recipe, a 64 x 128
frame on a 64-row map, where twenty vertices in at most 64 rows give shared rows, horizontal edges and den = 1 edges in
nearly every polygon.  One call of five frames with 0, 1, 64, 65 and 203 drops (nothing, one lane, a full wave, a wave and
a lane, three waves and a piece); every fifth drop lifted so that wrapping polygons take the list route inside the same
waves; a few drops pushed towards the map's seam column and its bottom row, where a vertex leaves the map.  (A vertex that
does leave it -- column We, row He -- lies within k_fov_vertices' own margins around the seam and the pole, so such a drop
is float64's and the list's, under the span rule there; tests/test_fov_walk_host.py walks vertices off the map under the
span rule directly.)
Rendered on the float colour route (want_composite=False) under RR_OPT_FOV_DDA 1 / 0 x RR_OPT_FOV_FILL_RULE 1 / 0 x
RR_OPT_FOV_ORDER 1 / 0: within a fill rule every output is the same bits whichever kernel made the spans and in whichever
order, and the default combination agrees with the numpy oracle."""
import itertools

import numpy as np
import pytest

import helpers as h
from oracle import render as orc
from test_gpu_fov_order import _lift

pytestmark = pytest.mark.gpu

H, W = 64, 128
COUNTS = (0, 1, 64, 65, 203)
KEYS = ('colour', 'status', 'mask', 'mask_i32', 'image_u8')


def _push(drops):
    """Drops 3, 8 and 13 (none of the lifted ones) of a frame that has them: far to the side and far down at their own depth,
    towards the seam column and the bottom row of the map."""
    for j, (sx, sy) in zip((3, 8, 13), ((-6.0, 0.0), (0.0, -4.0), (-6.0, -4.0))):
        if j < len(drops):
            for k in ('wps', 'wpe'):
                drops[k][j, 0] += abs(drops[k][j, 2]) * sx
                drops[k][j, 1] += abs(drops[k][j, 2]) * sy
    return drops


@pytest.fixture(scope="module")
def rendered(tmp_path_factory, built):
    sc = h.Scene(tmp_path_factory.mktemp('fov_walk'), H, W, 230, n_frames=len(COUNTS), seed0=4300)
    frames = []
    for i, n in enumerate(COUNTS):
        bg, env = sc.frame_inputs(i)
        drops = _push(_lift(sc.product_drops(i)[:n].copy()))
        frames.append(dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=drops))
    outs, launched = {}, {}
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        rh.profile(True)
        for dda, rule, order in itertools.product((1, 0), (1, 0), (1, 0)):
            rh.set_option(h.hb.RR_OPT_FOV_DDA, dda)
            rh.set_option(h.hb.RR_OPT_FOV_FILL_RULE, rule)
            rh.set_option(h.hb.RR_OPT_FOV_ORDER, order)
            rh.profile_reset()
            outs[dda, rule, order] = rh.render_frames(frames, want_composite=False, want_colour=True)
            launched[dda, rule, order] = rh.profile_read()
    finally:
        rh.close()
    return sc, frames, outs, launched


def test_the_walk_was_launched(rendered):
    """RR_OPT_FOV_DDA 1: the thread-per-drop route's own scopes (k_fov_vertices, k_fov_sort; the walk and the list share
    k_fov_spans'); 0: neither.  Most polygons are 20-gons (the walk's), some of every frame but the empty one wrap (the list's)."""
    sc, frames, outs, launched = rendered
    for (dda, rule, order), prof in launched.items():
        for scope in ('k_fov_vertices', 'k_fov_sort'):
            assert (prof.get(scope, (0, 0.0))[0] >= 1) == (dda == 1), (dda, rule, order, scope, prof)
        for scope in ('k_fov_spans', 'k_fov_sums'):
            assert prof.get(scope, (0, 0.0))[0] >= 1, (dda, rule, order, scope, prof)
    for fr, n in zip(frames, COUNTS):
        npts = np.array([len(orc.compute_fov_plane_points(d['wps'].copy(), d['wpe'].copy(), orc.RADIUS, orc.FOV_DEG, orc.N_FOV,
                                                          fr['env_xyY'].shape)) for d in fr['drops']], int)
        assert len(npts) == n
        if n > 1:
            assert (npts == orc.N_FOV).sum() > n // 2 and (npts == orc.N_FOV + 4).sum() >= 3, np.bincount(npts)
    assert (outs[1, 1, 1][4]['status'] == 0).sum() > COUNTS[4] // 2


@pytest.mark.parametrize("rule", [1, 0])
def test_same_bits_within_a_fill_rule(rendered, rule):
    sc, frames, outs, launched = rendered
    base = outs[1, rule, 1]
    for dda, order in ((1, 0), (0, 1), (0, 0)):
        for f, (a, b) in enumerate(zip(base, outs[dda, rule, order])):
            for k in KEYS:
                assert np.array_equal(a[k], b[k]), (rule, dda, order, f, k)


def test_the_fill_rules_differ(rendered):
    """(so that the comparison above is one of two different span sets, not of one)"""
    sc, frames, outs, launched = rendered
    assert any(not np.array_equal(a['colour'], b['colour']) for a, b in zip(outs[1, 1, 1], outs[1, 0, 1]))


def test_default_call_against_the_oracle(rendered):
    sc, frames, outs, launched = rendered
    textures, _ = sc.oracle_db()
    for f, (fr, out) in enumerate(zip(frames, outs[1, 1, 1])):
        ref = orc.render_drop_records(fr['bg'], fr['bg'], fr['env_xyY'], sc.omega, fr['drops'], textures, sc.ocam, faithful=True)
        assert np.array_equal(out['status'], ref['status']), f
        assert np.array_equal(out['mask'], ref['mask']) and np.array_equal(out['mask_i32'], ref['mask_i32']), f
        assert np.abs(out['image_u8'].astype(int) - ref['image_u8'].astype(int)).max() <= 1, f
