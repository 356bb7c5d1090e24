"""GPU tier: every defocus-blur route (tests/blur_routes.py) through the C ABI against the oracle, with failures localised to
the routes whose drops touch the differing pixels; the same drops inside a multi-frame batch; a frame past SLOW_CAP slow
drops compared whole; and rr_batch_counts against the classifier's counts, exactly."""
import numpy as np
import pytest

import blur_routes as br
import helpers as h

pytestmark = pytest.mark.gpu


def _frame_scene(tmp, particles, H, W):
    return h.Scene(tmp, H, W, 0, frames=[dict(id=0, t=2000, d=0, drops=particles)])


@pytest.fixture(scope='module')
def cases(built, tmp_path_factory):
    """name -> (scene, drops, classifier records, reference, what the reference is)."""
    out = {}
    for name, particles, H, W in (('catalogue', br.catalogue_particles(br.CATALOGUE, br.CAT_H, br.CAT_W), br.CAT_H, br.CAT_W),
                                  ('slow_cap', br.slow_cap_particles(300, 240, 320), 240, 320),
                                  ('boundary', br.catalogue_particles(br.BOUNDARY, br.CAT_H, br.CAT_W), br.CAT_H, br.CAT_W)):
        sc = _frame_scene(tmp_path_factory.mktemp(name), particles, H, W)
        bg, env = sc.frame_inputs(0)
        drops = sc.product_drops(0)
        if name == 'boundary':
            # the rendered side of RR_DROP_TOO_BIG is a ~2100 x 2100 padded tile filtered at radius 410: minutes of numpy.
            # The g++ build of the kernel arithmetic stands in (test_blur_routes_host puts it against the oracle on the rest)
            ref, what = h.emu_render(sc, bg, bg, env, drops), 'hostemu'
        else:
            ref, what = h.oracle_render(sc, 0, bg, bg, env, faithful=False), 'oracle'
        out[name] = (sc, drops, br.classify_drops(sc, drops), ref, what)
    return out


def _ctx(sc, **opts):
    rh = h.hb.RainHip(0)
    rh.set_streak_db(sc.db.streaks_light)
    rh.set_camera(sc.cam)
    for o, v in opts.items():
        rh.set_option(getattr(h.hb, o), v)
    return rh


def _frame(sc, drops):
    bg, env = sc.frame_inputs(0)
    return dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=drops)


@pytest.mark.parametrize('name', ['catalogue', 'slow_cap', 'boundary'])
def test_routes_match_reference(cases, name):
    sc, drops, recs, ref, what = cases[name]
    rh = _ctx(sc)
    try:
        out = rh.render_frames([_frame(sc, drops)])[0]
    finally:
        rh.close()
    br.check(out, ref, recs, '%s vs %s' % (name, what))
    if name == 'slow_cap':
        assert sum('beyond_cap' in r['flags'] for r in recs) > 0
    assert out['mask'].max() > 0


def _batch(sc, drops, recs):
    """[catalogue, empty, the catalogue's small drops, catalogue]: per-frame offsets of items, weight tables and wtab_big."""
    small = drops[[r['i'] for r in recs if r['route'] == 'small']]
    assert len(small) >= 3
    return [drops, np.zeros(0, h.hb.DROP_DTYPE), small, drops]


@pytest.mark.parametrize('tile_rows', [0, 2])
def test_multi_frame_batch_and_counts(cases, tile_rows):
    """The catalogue in frames 0 and 3 of a four-frame call equals the catalogue alone, bit for bit; every frame's
    rr_batch_counts [2] .. [6] equals the classifier's (RR_OPT_DEDUP 0: every drop renders its own raw tile)."""
    sc, drops, recs, ref, _ = cases['catalogue']
    rh = _ctx(sc, RR_OPT_DEDUP=0, RR_OPT_TILE_ROWS=tile_rows)
    try:
        alone = rh.render_frames([_frame(sc, drops)])[0]
        assert rh.batch_counts(0)[2:7] == br.expected_counts(recs), 'catalogue alone'
        batch = _batch(sc, drops, recs)
        outs = rh.render_frames([_frame(sc, d) for d in batch])
        counts = [rh.batch_counts(f)[2:7] for f in range(len(batch))]
    finally:
        rh.close()
    br.check(alone, ref, recs, 'catalogue alone (tile_rows %d)' % tile_rows)
    for f in (0, 3):
        for k in ('status', 'mask', 'mask_i32', 'image_u8', 'rainy_bg'):
            diff = outs[f][k] != alone[k]
            assert not diff.any(), 'frame %d of the batch: %s (%s)' % (
                f, k, diff.nonzero()[0][:8] if k == 'status' else br.routes_touching(recs, diff.reshape(diff.shape[:2] + (-1,)).any(axis=2)))
    assert outs[1]['mask'].max() == 0
    srecs = br.classify_drops(sc, batch[2])
    assert all(r['route'] == 'small' for r in srecs)
    bg, env = sc.frame_inputs(0)
    br.check(outs[2], h.emu_render(sc, bg, bg, env, batch[2]), srecs, 'small-only frame vs hostemu')
    for f, d in enumerate(batch):
        assert counts[f] == br.expected_counts(br.classify_drops(sc, d)), 'frame %d of the batch' % f


@pytest.mark.parametrize('tile_rows', [0, 2])
def test_counts_past_slow_cap(cases, tile_rows):
    for name in ('slow_cap', 'boundary'):
        sc, drops, recs, _, _ = cases[name]
        rh = _ctx(sc, RR_OPT_DEDUP=0, RR_OPT_TILE_ROWS=tile_rows)
        try:
            rh.render_frames([_frame(sc, drops)])
            assert rh.batch_counts(0)[2:7] == br.expected_counts(recs), name
        finally:
            rh.close()
