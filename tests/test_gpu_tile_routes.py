"""GPU tier: every raw-tile route (tests/tile_routes.py) through the C ABI against the reference -- the catalogue frames under the
default options and, with tile sharing off, under RR_OPT_TILE_ROWS 0 / 1 / 2 and two share counts, each compared with the oracle
(not with another route) and with rr_batch_counts as the classifier predicts them; one database per side of each texture limit;
the list-scheduling shapes (only Big tiles, no rows tile, one, three, forty in one bucket, empty frames around the catalogue) as
one call against the frames rendered alone; and the tile sharing of k_dedup against the raw-tile keys of the host build.
A failure names the routes and flags of the entries whose footprints hold the differing pixels."""
import numpy as np
import pytest

import helpers as h
import tile_routes as tr

pytestmark = pytest.mark.gpu

MODES = {'rows_0': dict(RR_OPT_TILE_ROWS=0), 'rows_1': dict(RR_OPT_TILE_ROWS=1), 'rows_2': dict(RR_OPT_TILE_ROWS=2),
         'rows_2_shares_1': dict(RR_OPT_TILE_ROWS=2, RR_OPT_ROWS_SHARES=1), 'rows_2_shares_8': dict(RR_OPT_TILE_ROWS=2, RR_OPT_ROWS_SHARES=8)}
KEYS = ('status', 'mask', 'mask_i32', 'image_u8', 'rainy_bg')


def _case(tmp, drops, **db):
    """(scene, packed drops, records, oracle's frame)."""
    sc = tr.scene(tmp, drops, **db)
    packed = tr.frame_drops(sc, len(drops))
    bg, env = sc.frame_inputs(0)
    return sc, packed, tr.classify_drops(sc, packed), h.oracle_render(sc, 0, bg, bg, env, faithful=False)


@pytest.fixture(scope='module')
def catalogue(built, tmp_path_factory):
    return {fam: _case(tmp_path_factory.mktemp(fam), [e[3:] for e in tr.CATALOGUE[fam]]) for fam in tr.FAMILIES}


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


def _render(sc, frames, **opts):
    """(outputs, rr_batch_counts) of one call."""
    rh = _ctx(sc, **opts)
    try:
        outs = rh.render_frames([_frame(sc, d) for d in frames])
        return outs, [rh.batch_counts(f) for f in range(len(frames))]
    finally:
        rh.close()


def _same_bits(a, b, recs, tag):
    for k in KEYS:
        diff = a[k] != b[k]
        assert not diff.any(), '%s: %s (%s)' % (tag, k, diff.nonzero()[0][:8] if k == 'status' else
                                                tr.routes_touching(recs, diff.reshape(diff.shape[:2] + (-1,)).any(axis=2)))


@pytest.mark.parametrize('fam', tr.FAMILIES)
def test_catalogue_matches_reference(catalogue, fam):
    sc, drops, recs, ref = catalogue[fam]
    outs, _ = _render(sc, [drops])
    tr.check(outs[0], ref, recs, '%s vs oracle' % fam)
    assert outs[0]['mask'].max() > 0


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('fam', tr.FAMILIES)
def test_every_route_matches_reference(catalogue, fam, mode):
    """Each setting against the oracle, not against another setting: a defect the routes share does not pass.  RR_OPT_DEDUP 0:
    every drop renders its own tile, and the work lists hold what the classifier says."""
    sc, drops, recs, ref = catalogue[fam]
    outs, counts = _render(sc, [drops], RR_OPT_DEDUP=0, **MODES[mode])
    tile_rows = MODES[mode]['RR_OPT_TILE_ROWS']
    assert tr.counts_of(counts[0]) == tr.expected_counts(recs, tile_rows), '%s %s: rr_batch_counts [0], [1], [5], [6]' % (fam, mode)
    tr.check(outs[0], ref, recs, '%s %s vs oracle' % (fam, mode))


@pytest.mark.parametrize('k', range(len(tr.TEXTURE_LIMIT_DBS) + 1))
def test_texture_limits(built, tmp_path, k):
    if k < len(tr.TEXTURE_LIMIT_DBS):
        name, heights, width, route, drops = tr.TEXTURE_LIMIT_DBS[k]
        routes = [route] * len(drops)
    else:
        name, heights, width, entries = tr.SCALE_X_DB
        drops, routes = [e[3] for e in entries], [e[1] for e in entries]
    sc, packed, recs, ref = _case(tmp_path, drops, tex_heights=heights, tex_width=width)
    assert [r['route'] for r in recs] == routes, name
    outs, counts = _render(sc, [packed], RR_OPT_DEDUP=0)
    assert tr.counts_of(counts[0]) == tr.expected_counts(recs, 2), name
    tr.check(outs[0], ref, recs, '%s vs oracle' % name)
    outs, _ = _render(sc, [packed])
    tr.check(outs[0], ref, recs, '%s (default options) vs oracle' % name)
    assert outs[0]['mask'].max() > 0


def _shape_frames(tmp, catalogue, name):
    """[(scene, packed drops, records, reference) or None for an empty frame] of LIST_SHAPES[name]."""
    shape, out = tr.LIST_SHAPES[name], []
    for k, fr in enumerate(shape['frames']):
        if isinstance(fr, str):
            out.append(catalogue[fr])
        elif not fr:
            out.append(None)
        elif shape.get('one_texture'):
            sc = tr.scene(tmp / ('f%d' % k), fr)
            packed = tr.frame_drops(sc, len(fr))
            packed['tex_index'] = packed['tex_index'][0]
            bg, env = sc.frame_inputs(0)
            out.append((sc, packed, tr.classify_drops(sc, packed), h.emu_render(sc, bg, bg, env, packed)))     # (the host build: the
        else:                                                                                                   #  oracle draws its own textures)
            out.append(_case(tmp / ('f%d' % k), fr))
    return out


@pytest.mark.parametrize('dedup', [0, 1])
@pytest.mark.parametrize('name', list(tr.LIST_SHAPES))
def test_list_shapes(catalogue, tmp_path, name, dedup):
    """One call per shape: every frame equals the same frame rendered alone, bit for bit, and that equals the reference."""
    frames = _shape_frames(tmp_path, catalogue, name)
    sc = next(f[0] for f in frames if f is not None)
    empty = np.zeros(0, h.hb.DROP_DTYPE)
    outs, counts = _render(sc, [empty if f is None else f[1] for f in frames], RR_OPT_DEDUP=dedup)
    for k, f in enumerate(frames):
        if f is None:
            assert outs[k]['mask'].max() == 0 and tr.counts_of(counts[k]) == [0, 0, 0, 0], (name, k)
            continue
        _, drops, recs, ref = f
        alone, _ = _render(sc, [drops], RR_OPT_DEDUP=dedup)
        _same_bits(outs[k], alone[0], recs, '%s frame %d of the call vs alone' % (name, k))
        tr.check(alone[0], ref, recs, '%s frame %d alone vs reference' % (name, k))
        assert alone[0]['mask'].max() > 0
        if dedup == 0:
            assert tr.counts_of(counts[k]) == tr.expected_counts(recs, 2), (name, k)
    routes = {r['route'] for f in frames if f is not None for r in f[2] if r['live']}
    if name == 'only_big':
        assert routes == {'big_lds', 'big'}
    elif name == 'only_rot_int':
        assert routes == {'rot_int'}
    elif name in ('one_rows_tile', 'three_rows_tiles', 'forty_copies'):
        assert routes == {'rows'} and sum(len(f[2]) for f in frames) == {'one_rows_tile': 1, 'three_rows_tiles': 3, 'forty_copies': 40}[name]


def test_tile_sharing(catalogue, tmp_path):
    """k_dedup: the catalogue frame twice in one call renders every tile once -- rr_batch_counts [7] over the call is the number
    of live drops; forty copies of one streak with one texture share what their raw-tile keys say; the same bits without sharing."""
    sc, drops, recs, ref = catalogue['small']
    n_live = sum(r['live'] for r in recs)
    assert tr.expected_shared(sc, [drops]) == 0                # no two entries have one raw tile
    outs, counts = _render(sc, [drops, drops])
    assert sum(c[7] for c in counts) == tr.expected_shared(sc, [drops, drops]) == n_live
    plain, _ = _render(sc, [drops, drops], RR_OPT_DEDUP=0)
    for k in (0, 1):
        _same_bits(outs[k], plain[k], recs, 'catalogue twice, frame %d: shared vs own tiles' % k)
        tr.check(outs[k], ref, recs, 'catalogue twice, frame %d vs oracle' % k)
    (sc, drops, recs, ref), = _shape_frames(tmp_path, catalogue, 'forty_copies')
    want = tr.expected_shared(sc, [drops])
    assert want >= 30, want                                    # (streaks shifted by whole pixels: nearly all one tile)
    outs, counts = _render(sc, [drops])
    assert counts[0][7] == want
    plain, counts = _render(sc, [drops], RR_OPT_DEDUP=0)
    assert counts[0][7] == 0
    _same_bits(outs[0], plain[0], recs, 'forty copies: shared vs own tiles')
    tr.check(outs[0], ref, recs, 'forty copies vs the host build')
