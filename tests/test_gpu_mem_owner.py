"""GPU tier: what a context holds (rr_debug_mem: device blocks, their bytes, pinned blocks, their bytes) is settled by the
first batch of a kind -- the same batch again changes nothing, a larger batch or another frame size REPLACES blocks and adds
none, the pipeline slots settle after their first batch, and a new context after close() arrives at the same numbers.  One
context, the smoke scene's size; no free-memory query of the (shared) device."""
import numpy as np
import pytest

import helpers as h

pytestmark = pytest.mark.gpu


def _frame(sc, i):
    bg, env = sc.frame_inputs(i)
    return dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=sc.product_drops(i))


def _fresh(sc):
    rh = h.hb.RainHip(0)
    rh.set_streak_db(sc.db.streaks_light)
    rh.set_camera(sc.cam)
    return rh


def test_context_memory_is_settled_replaced_and_released(tmp_path, built):
    sc = h.Scene(tmp_path / 'a', 96, 160, 120, n_frames=3)
    small = h.Scene(tmp_path / 'b', 64, 96, 60)
    frames = [_frame(sc, i) for i in range(3)]
    rh = _fresh(sc)
    try:
        first = rh.render_frames(frames[:1])[0]
        m1 = rh.debug_mem()
        print('after the first render:', m1)
        assert m1[0] > 0 and m1[1] > 0 and m1[2] > 0 and m1[3] > 0
        # the same batch twice
        again = rh.render_frames(frames[:1])[0]
        assert rh.debug_mem() == m1
        assert np.array_equal(again['mask'], first['mask']) and np.array_equal(again['image_u8'], first['image_u8'])
        # growth: more frames, then another frame size -- both walk the paths the first render took, so no block is new
        rh.render_frames(frames)
        m3 = rh.debug_mem()
        print('after three frames:', m3)
        assert m3[0] <= m1[0] and m3[1] > m1[1]
        rh.set_streak_db(small.db.streaks_light)
        rh.set_camera(small.cam)
        rh.render_frames([_frame(small, 0)])
        ms = rh.debug_mem()
        print('after a 64 x 96 frame:', ms)
        assert ms[0] <= m1[0]
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        back = rh.render_frames(frames[:1])[0]
        assert np.array_equal(back['mask'], first['mask']) and np.array_equal(back['image_u8'], first['image_u8'])
        assert rh.debug_mem()[0] <= m1[0]

        # pipeline: one batch on slot 0 and one on slot 1; repeated, nothing moves
        def round_trip():
            outs = [dict(image_u8=np.zeros((96, 160, 3), np.uint8), mask=np.zeros((96, 160)),
                         status=np.zeros(len(frames[k]['drops']), np.int32)) for k in range(2)]
            for slot in range(2):
                rh.pipeline_submit(slot, [frames[slot]], [outs[slot]])
            for slot in range(2):
                while not rh.pipeline_wait(slot):               # (arena regrown: the batch again)
                    rh.pipeline_submit(slot, [frames[slot]], [outs[slot]])
            return outs
        outs = round_trip()
        mp = rh.debug_mem()
        print('after the pipeline slots:', mp)
        assert np.array_equal(outs[0]['mask'], first['mask'])
        outs2 = round_trip()
        assert rh.debug_mem() == mp
        for o, o2 in zip(outs, outs2):
            assert np.array_equal(o['mask'], o2['mask']) and np.array_equal(o['image_u8'], o2['image_u8'])
    finally:
        rh.close()
    # close, then create, render and close twice more: the same four numbers after the same first render
    for _ in range(2):
        rh = _fresh(sc)
        try:
            out = rh.render_frames(frames[:1])[0]
            assert rh.debug_mem() == m1
            assert np.array_equal(out['mask'], first['mask']) and np.array_equal(out['image_u8'], first['image_u8'])
        finally:
            rh.close()
