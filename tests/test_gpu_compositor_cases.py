"""GPU tier: the compositor catalogues (tests/compositor_cases.py) through the C ABI on every route of the compositor, against
the references the CPU tier put on trial (tests/test_compositor_cases_host.py): the oracle, and the host build for the two
tables the oracle would take minutes for.  A failure names the catalogue entries, the screen tile, the wave quadrant and the
lane's pixel of the differing pixels."""
import numpy as np
import pytest

import compositor_cases as cc
import helpers as h

pytestmark = pytest.mark.gpu

# name -> (rr_set_option settings, want_composite, the geometry of the compositor that runs)
CONFIGS = {
    'default': ({}, False, cc.GEOM32),                               # k_composite32, 16-bit codes, k_finalize16
    'composite': ({}, True, cc.GEOM64),                              # k_composite, k_finalize; rainy_bg within 1e-9
    'composite_f64': (dict(RR_OPT_COMPOSITE_F64=1), False, cc.GEOM64),
    'wild_pixels': (dict(RR_OPT_WILD_PIXELS=1), False, cc.GEOM32),   # k_pad_visits, float composite, k_finalize; inputs in [0, 1]: same output
    'one_stream': (dict(RR_OPT_COLOUR_STREAM=0), False, cc.GEOM32),
}
CATALOGUES = {'seams': ('seams_low', 'seams_high'), 'lengths': ('lengths',), 'indices': ('indices', 'segment'),
              'shapes': tuple(s[0] for s in cc.SHAPES) + ('wide',)}


def _wall(c):
    """A scene-depth wall between the two depths of a stack's drops (6.0 and 6.5 m), open on four rows of sixteen."""
    d = np.full((c.H, c.W), 6.25)
    d[np.arange(c.H) % 16 >= 12] = 100.0
    return d


@pytest.fixture(scope='module')
def cat(built, tmp_path_factory):
    """name -> Case with case.ref (the reference) and case.ref_is ('oracle' / 'host build')."""
    tpl = cc.Templates(tmp_path_factory.mktemp('tpl'))
    cases = [cc.seams(tmp_path_factory.mktemp('sl'), tpl, 'low'), cc.seams(tmp_path_factory.mktemp('sh'), tpl, 'high'),
             cc.lengths(tmp_path_factory.mktemp('le'), tpl), cc.indices(tmp_path_factory.mktemp('in'), tpl),
             cc.segment(tmp_path_factory.mktemp('sg'), tpl)] + cc.shapes(lambda n: tmp_path_factory.mktemp(n), tpl)
    out = {}
    for c in cases:
        if c.name == 'segment':
            # BIN_SEG + 40 rendering records are a minute of numpy: the host build, which the CPU tier holds to the oracle
            # around the segment boundary
            c.ref, c.ref_is = c.emu(), 'host build'
        elif c.name == 'indices':
            # the oracle on the rendering records alone (the CPU tier: the host build on the whole table gives the same)
            keep = np.setdiff1d(np.arange(len(c.drops)), c.filler)
            c.ref, c.ref_is = c.oracle(c.drops[keep]), 'oracle'
            status = np.zeros(len(c.drops), np.int32)
            status[keep] = c.ref['status']
            c.ref['status'] = status
        else:
            c.ref, c.ref_is = c.oracle(), 'oracle'
        out[c.name] = c
    return out


def _ctx(c, **opts):
    rh = h.hb.RainHip(0)
    rh.set_streak_db(c.scene.db.streaks_light)
    rh.set_camera(c.scene.cam)
    for o, v in opts.items():
        rh.set_option(getattr(h.hb, o), v)
    return rh


def _render(c, frames, want_composite=False, **opts):
    rh = _ctx(c, **opts)
    try:
        return rh.render_frames(frames, want_composite=want_composite)
    finally:
        rh.close()


@pytest.mark.parametrize('config', list(CONFIGS))
@pytest.mark.parametrize('catalogue', list(CATALOGUES))
def test_catalogue_matches_reference(cat, catalogue, config):
    opts, want, geom = CONFIGS[config]
    for name in CATALOGUES[catalogue]:
        c = cat[name]
        out = _render(c, [c.frame()], want, **opts)[0]
        cc.check(out, c.ref, c, '%s vs %s' % (config, c.ref_is), geom)
        assert out['mask'].max() > 0


def test_wide_frame_is_binned_by_k_bin(cat):
    """What sends the 4112-wide frame of `shapes` to k_bin is its 65 coarse tiles per row (rr_render's `ctiles_x <= 64`); the
    library's profile gives both binning kernels the one scope name, so the launch is inferred from that line.  Drops lie in
    the 64th and 65th coarse tile and one box across x = 4096."""
    c = cat['wide']
    assert -(-c.W // cc.CTILE) == 65 > cc.BIN_ROWS_MAX_CT
    keep, boxes = cc.listed_drops(c.scene, c.drops, c.ref['status'])
    wl = cc.work_lists(c.H, c.W, keep, boxes, cc.GEOM32)
    assert len(wl['coarse'][(0, 63)]) > 6 and len(wl['coarse'][(0, 64)]) > 6 and any(boxes[i][0] < 4096 < boxes[i][2] for i in keep)


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_seams_with_narrow_image_inputs(cat, dtype):
    """The odd-width frame with uint8 (value / 255) and float32 images: the raw-word pixel loads of k_composite32's prologue."""
    c = cat['seams_low']
    bg = np.round(c.bg * 255).astype(np.uint8) if dtype == 'uint8' else c.bg.astype(np.float32)
    ref = c.oracle(bg=bg.astype(np.float64) / 255.0 if dtype == 'uint8' else bg.astype(np.float64))
    for config in ('default', 'composite'):
        opts, want, geom = CONFIGS[config]
        out = _render(c, [c.frame(bg=bg)], want, **opts)[0]
        cc.check(out, ref, c, '%s images, %s vs oracle' % (dtype, config), geom)


@pytest.mark.parametrize('config', ['default', 'composite'])
def test_batch_of_catalogues(cat, config):
    """seams, empty, lengths, seams in one call.  The frames of a call share one size (test_frames_of_a_call_share_one_size), so
    all four are the frame of `lengths`, with the seams table in frames 0 and 3: the same bits as that table alone, and
    frame 2 the same bits as `lengths` alone -- per-frame offsets of lists, counts, records and tile sums."""
    opts, want, geom = CONFIGS[config]
    c, s = cat['lengths'], cat['seams_high']
    rh = _ctx(c, **opts)
    try:
        seams_alone = rh.render_frames([c.frame(s.drops)], want_composite=want)[0]
        lengths_alone = rh.render_frames([c.frame()], want_composite=want)[0]
        outs = rh.render_frames([c.frame(s.drops), c.frame(np.zeros(0, h.hb.DROP_DTYPE)), c.frame(), c.frame(s.drops)], want_composite=want)
    finally:
        rh.close()
    cc.check(lengths_alone, c.ref, c, 'lengths alone (%s)' % config, geom)
    cc.check(seams_alone, c.emu(s.drops), s, 'seams on the frame of lengths vs host build (%s)' % config, geom)
    for f, alone, case in ((0, seams_alone, s), (2, lengths_alone, c), (3, seams_alone, s)):
        for k in ('status', 'mask', 'mask_i32', 'image_u8') + (('rainy_bg',) if want else ()):
            diff = outs[f][k] != alone[k]
            assert not diff.any(), 'frame %d of the batch: %s %s' % (
                f, k, diff.nonzero()[0][:8] if k == 'status' else cc.where(case, diff.reshape(diff.shape[:2] + (-1,)).any(axis=2), geom))
    assert outs[1]['mask'].max() == 0 and seams_alone['mask'].max() > 0


def test_frames_of_a_call_share_one_size(cat):
    """The library refuses a call whose frames differ in size: why the batch above puts both tables on one frame."""
    c, s = cat['lengths'], cat['seams_low']
    rh = _ctx(c)
    try:
        with pytest.raises(RuntimeError):
            rh.render_frames([s.frame(), c.frame()], want_composite=False)
    finally:
        rh.close()


@pytest.mark.parametrize('config', ['default', 'composite'])
def test_depth_wall_hides_every_second_drop(cat, config):
    """RR_OPT_DEPTH_OCCLUSION: the drops of a stack alternate between 6.0 and 6.5 m, the wall stands at 6.25 m (and is open on
    four rows of sixteen: hidden and visible pixels in one wave).  Against the oracle's scene_depth."""
    opts, want, geom = CONFIGS[config]
    c = cat['lengths']
    wall = _wall(c)
    if not hasattr(c, 'ref_wall'):
        c.ref_wall = c.oracle(scene_depth=wall)
    assert (c.ref_wall['mask'] != c.ref['mask']).any() and c.ref_wall['mask'].max() > 10
    out = _render(c, [c.frame(depth=wall)], want, RR_OPT_DEPTH_OCCLUSION=1, **opts)[0]
    cc.check(out, c.ref_wall, c, 'depth wall, %s vs oracle' % config, geom)


def test_one_wave_on_the_literal_blend(cat):
    """One out-of-range pixel under an overlap group sends its wave of k_composite32 to the float64 blend_pixel, entry by entry.
    The reference is the float64 compositor of the same frame at the bars of test_colour_stream_and_composite_codes."""
    c = cat['seams_low']
    bg = c.bg.copy()
    bg[48, 24] = (1.5, -0.5, 2.0)                         # under `quad32`: tile (1, 1) of 16 x 32, its lower right wave
    rh = _ctx(c)
    try:
        out = rh.render_frames([c.frame(bg=bg)], want_composite=False)[0]
        f64 = rh.render_frames([c.frame(bg=bg)], want_composite=True)[0]
    finally:
        rh.close()
    for k in ('status', 'mask', 'mask_i32'):
        diff = out[k] != f64[k]
        assert not diff.any(), '%s: %s' % (k, cc.where(c, diff, cc.GEOM32) if k != 'status' else diff.nonzero()[0][:8])
    diff = (np.abs(out['image_u8'].astype(int) - f64['image_u8'].astype(int)) > 1).any(axis=2)
    assert not diff.any(), 'image_u8: %s' % cc.where(c, diff, cc.GEOM32)
    assert np.array_equal(out['mask'], c.ref['mask'])
