"""GPU tier: the order in which k_fov_dda's waves take a frame's drops (RR_OPT_FOV_ORDER; k_fov_vertices -> k_fov_sort ->
k_fov_dda, span columns indexed by slot).  One call of four frames on a 64-row map with 0, 1, 65 and 203 drops -- an empty
frame, a single slot, a wave and one lane, three waves and a piece -- in which every fifth drop is lifted out of the narrow
view so that its polygon contains a pole of the map (most of them: 24 vertices, the k_fov_spans list route, whose spans
go to the drop's slot through the inverse permutation), and two drops of the largest frame are copies of a third, one of
k_fov_dda's (equal sort keys: ties).
Rendered on the float colour route (no float64 composite asked for: want_composite=False), the only one that launches
these kernels; the library's own launch counts say that it was taken.  Sorted and in table order every output is the same
bits, and the sorted call agrees with the numpy oracle like the whole-frame parity tests."""
import numpy as np
import pytest

import helpers as h
from oracle import render as orc

pytestmark = pytest.mark.gpu

H, W = 64, 128
COUNTS = (0, 1, 65, 203)


def _lift(drops):
    """Every fifth drop (and the frame's only one): moved up or down by 40 .. 19 degrees of elevation at its own depth.
    The 165-degree cone around the drop's direction, cut with the 10 m sphere from a metre or two in front of the
    camera, then contains a pole of the map from about 20 degrees on: the polygon wraps."""
    for j in range(0, len(drops), 5):
        ang = np.deg2rad((40.0 - (j // 5) % 8 * 3.0) * (-1 if (j // 5) % 2 else 1))
        for k in ('wps', 'wpe'):
            drops[k][j, 1] += abs(drops[k][j, 2]) * np.tan(ang)
    return drops


@pytest.fixture(scope="module")
def rendered(tmp_path_factory, built):
    sc = h.Scene(tmp_path_factory.mktemp('fov_order'), H, W, 230, n_frames=len(COUNTS), seed0=4100)
    frames = []
    for i, n in enumerate(COUNTS):
        bg, env = sc.frame_inputs(i)
        drops = _lift(sc.product_drops(i)[:n].copy())
        if n > 150:                                    # identical records: next to each other and a wave apart
            drops[101] = drops[102]
            drops[7] = drops[102]
        frames.append(dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=drops))
    outs, launched = {}, {}
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        rh.profile(True)
        for order in (1, 0):
            rh.set_option(h.hb.RR_OPT_FOV_ORDER, order)
            rh.profile_reset()
            # (a float64 composite would put the whole colour branch in float64: k_fov_spans for every drop, no order)
            outs[order] = rh.render_frames(frames, want_composite=False, want_colour=True)
            launched[order] = rh.profile_read()
    finally:
        rh.close()
    return sc, frames, outs, launched


def test_both_routes_occur(rendered):
    """The library launched the thread-per-drop route's kernels in both calls (its timing scopes: k_fov_vertices, k_fov_sort,
    and k_fov_spans for the walk and the list), and on that route a polygon's size decides which kernel makes its spans --
    npts of the reference's polygon: 20 vertices (k_fov_dda walks them) and 24 (a wrap: the list, k_fov_spans)."""
    sc, frames, outs, launched = rendered
    for order in (1, 0):
        for scope in ('k_fov_vertices', 'k_fov_sort', 'k_fov_spans', 'k_fov_sums'):
            assert launched[order].get(scope, (0, 0.0))[0] >= 1, (order, scope, launched[order])
    for fr, n in zip(frames, COUNTS):
        npts = np.array([len(orc.compute_fov_plane_points(d['wps'].copy(), d['wpe'].copy(), orc.RADIUS, orc.FOV_DEG, orc.N_FOV,
                                                          fr['env_xyY'].shape)) for d in fr['drops']], int)
        assert len(npts) == n
        if n == 1:
            assert npts[0] == orc.N_FOV + 4           # the lonely drop takes the list route: slot 0 through the inverse
        if n > 1:
            assert (npts == orc.N_FOV).sum() > n // 2 and (npts == orc.N_FOV + 4).sum() >= 3, np.bincount(npts)
    assert (outs[1][3]['status'] == 0).sum() > COUNTS[3] // 2


def test_sorted_and_table_order_are_the_same_bits(rendered):
    sc, frames, outs, launched = rendered
    for f, (a, b) in enumerate(zip(outs[1], outs[0])):
        for k in ('image_u8', 'mask', 'mask_i32', 'status', 'colour'):
            assert np.array_equal(a[k], b[k]), (f, k)
    big = outs[1][3]
    assert np.array_equal(big['colour'][102], big['colour'][101]) and np.array_equal(big['colour'][102], big['colour'][7])
    assert big['status'][102] == big['status'][101] == big['status'][7]


def test_sorted_call_against_the_oracle(rendered):
    sc, frames, outs, launched = rendered
    textures, _ = sc.oracle_db()
    for f, (fr, out) in enumerate(zip(frames, outs[1])):
        ref = orc.render_drop_records(fr['bg'], fr['bg'], fr['env_xyY'], sc.omega, fr['drops'], textures, sc.ocam, faithful=True)
        assert np.array_equal(out['status'], ref['status']), f
        assert np.array_equal(out['mask'], ref['mask']) and np.array_equal(out['mask_i32'], ref['mask_i32']), f
        assert np.abs(out['image_u8'].astype(int) - ref['image_u8'].astype(int)).max() <= 1, f
