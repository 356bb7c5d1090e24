"""GPU tier: how the defocus blur writes finished tiles.  The catalogue of tests/blur_store_shape.py -- every branch of the
column passes of k_blur_small and k_blur_fused_dma, every remainder of the tile width against the four-column block, bands,
split drops, 2-D sub-tiles with a narrow last column, each blurred drop under an in-focus neighbour whose raw tile is next
in the arena -- through the C ABI against the g++ build of the kernel arithmetic (pinned to the oracle by
tests/test_blur_store_shape_host.py): statuses equal, both masks bit-exact, image within 1 LSB.  And the same catalogue as
frames 0 and 2 of a three-frame call with an empty frame between, bit-equal to the single-frame render."""
import numpy as np
import pytest

import blur_routes as br
import blur_store_shape as ss
import helpers as h

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def case(built, tmp_path_factory):
    sc = h.Scene(tmp_path_factory.mktemp('store_shape'), ss.H, ss.W, 0, frames=[dict(id=0, t=2000, d=0, drops=ss.particles())])
    bg, env = sc.frame_inputs(0)
    drops = sc.product_drops(0)
    assert len(drops) == len(ss.entries())
    recs = br.classify_drops(sc, drops)
    ref = h.emu_render(sc, bg, bg, env, drops)
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        frame = dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=drops)
        alone = rh.render_frames([frame])[0]
        batch = rh.render_frames([frame, dict(frame, drops=np.zeros(0, h.hb.DROP_DTYPE)), frame])
    finally:
        rh.close()
    return recs, ref, alone, batch


def test_catalogue_reaches_every_class(case):
    recs = case[0]
    reached = ss.classes(recs)
    assert not [k for k in ss.REQUIRED if not reached.get(k)], reached
    assert all(recs[k]['r1'] > 0 and recs[k + 1]['route'] == 'no_blur' and recs[k + 1]['live'] for k in range(0, len(recs), 2))


def test_finished_tiles_match_reference(case):
    recs, ref, alone, _ = case
    br.check(alone, ref, recs, 'store-shape catalogue vs hostemu')
    assert alone['mask'].max() > 0


def test_same_frame_inside_a_batch(case):
    recs, _, alone, batch = case
    assert len(batch) == 3 and batch[1]['mask'].max() == 0
    for f in (0, 2):
        for k in ('status', 'mask', 'mask_i32', 'image_u8', 'rainy_bg'):
            diff = batch[f][k] != alone[k]
            assert not diff.any(), 'frame %d of the batch: %s (%s)' % (
                f, k, diff.nonzero()[0][:8] if k == 'status' else br.routes_touching(recs, diff.reshape(diff.shape[:2] + (-1,)).any(axis=2)))
