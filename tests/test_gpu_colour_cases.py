"""GPU tier: the colour catalogue (tests/colour_cases.py) through the C ABI with want_colour=True, per drop against the float64
reference the CPU tier put on trial (tests/test_colour_cases_host.py).

Float route (no float64 composite asked for -- what main.py, bench.py and RainAugment run): the library's launch counts say
which kernels ran; statuses equal the reference's; a drop that is not composited has K = 0 exactly; every composited drop's
(x, y, Yg) = unmix(K) lies within rounding_bound of the reference.  Exceptions only for drops whose float polygon truncates
to another texel on the device (its atan2f / sqrtf are not the host's): at most 1 % of a case's composited drops (3 below
300), each within the bound of the reference on a polygon with ONE vertex moved ONE texel (colour_cases.Case.explain).
Float64 routes (a float64 composite; RR_OPT_FOV_F32 0): |K - reference| <= 1e-9 max|K|.  Every check prints its figures
(`colour-accuracy ...`) before it asserts."""
import numpy as np
import pytest

import colour_cases as col
import helpers as h

pytestmark = pytest.mark.gpu

FAST_FLOAT = ('k_fov_vertices', 'k_fov_sort', 'k_fov_spans', 'k_fov_sums')


@pytest.fixture(scope='module')
def cat(built, tmp_path_factory):
    base = col.Base(lambda n: tmp_path_factory.mktemp(n))
    return col.build(base)


class Ctx:
    """One library context for a group of cases; options are switched between calls and put back."""

    def __init__(self, base):
        self.rh = h.hb.RainHip(0)
        self.rh.set_streak_db(base.scene.db.streaks_light)
        self.rh.profile(True)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.rh.close()

    def render(self, case, frames, route='f32', **opts):
        """route: 'f32' the float route, 'f64c' a float64 composite, 'f64o' RR_OPT_FOV_F32 0.  Returns (outs, launch counts)."""
        rh = self.rh
        rh.set_camera(case.cam)
        opts = dict(opts)
        if route == 'f64o':
            opts['RR_OPT_FOV_F32'] = 0
        defaults = dict(RR_OPT_FOV_F32=2, RR_OPT_FOV_DROPS_PER_THREAD=0, RR_OPT_FOV_ORDER=1, RR_OPT_FOV_DDA=1, RR_OPT_COLOUR_STREAM=1,
                        RR_OPT_FOV_FILL_RULE=1)
        assert set(opts) <= set(defaults), opts
        try:
            for o, v in opts.items():
                rh.set_option(getattr(h.hb, o), v)
            rh.profile_reset()
            outs = rh.render_frames(frames, want_composite=route == 'f64c', want_colour=True)
            return outs, rh.profile_read()
        finally:
            for o in opts:
                rh.set_option(getattr(h.hb, o), defaults[o])


def _launched(prof, scopes, tag):
    for s in scopes:
        assert prof.get(s, (0, 0.0))[0] >= 1, (tag, s, sorted(prof))


def check_float(case, out, tag, n=None, rule=1):
    n = case.n if n is None else n
    r = case.ref(rule)
    comp = r['composited'][:n]
    assert np.array_equal(out['status'], r['status'][:n]), (tag, np.nonzero(out['status'] != r['status'][:n])[0][:8])
    K = out['colour']
    assert K.shape == (n, 3) and not K[~comp].any(), (tag, 'K of a drop that is not composited')
    got = col.unmix(K)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(comp[:, None], np.abs(got - r['xyY'][:n]) / r['bound'][:n], 0.0)
    bad = np.nonzero(~(ratio <= 1.0).all(axis=1))[0]
    cap = 3 if comp.sum() < 300 else int(0.01 * comp.sum())
    inside = np.delete(ratio, bad, axis=0)
    print('colour-accuracy %s n=%d composited=%d largest error / bound=%.3f largest bound (x y Yg, relative)=%s exceptions=%d cap=%d'
          % (tag, n, comp.sum(), inside.max() if inside.size else 0.0,
             np.array2string((r['bound'][:n][comp] / np.abs(r['xyY'][:n][comp])).max(axis=0) if comp.any() else np.zeros(3), precision=2), len(bad), cap))
    assert len(bad) <= cap, (tag, 'exceptions', len(bad), cap, bad[:10], ratio[bad[:10]])
    for i in bad:
        assert case.explain(int(i), got[i], rule) is not None, (tag, 'drop %d: no polygon one vertex and one texel away explains it' % i,
                                                                 got[i], r['xyY'][i], ratio[i])


def check_f64(case, out, tag, n=None, rule=1):
    n = case.n if n is None else n
    r = case.ref(rule)
    assert np.array_equal(out['status'], r['status'][:n]), tag
    err = np.abs(out['colour'] - r['K'][:n]).max() if n else 0.0
    scale = np.abs(r['K'][:n]).max() if n else 1.0
    print('colour-accuracy %s n=%d float64 largest |K - reference| / max|K|=%.3g' % (tag, n, err / scale))
    assert err <= 1e-9 * scale, (tag, err / scale)


@pytest.mark.parametrize('env', ['f32', 'f64'])
def test_widths_on_the_float_route(cat, env):
    """Every width class (idle waves, the odd width's last column, one pass and two, the widest map of the fast path), the map as
    float32 and as float64, under the 165- and the 60-degree cone; then every drops-per-thread instance on a one-pass and a
    two-pass width."""
    env32 = env == 'f32'
    with Ctx(next(iter(cat.values())).base) as ctx:
        for He, We in col.WIDTHS:
            for cone in (165, 60):
                c = cat[col.width_name(He, We, cone, env32)]
                outs, prof = ctx.render(c, [c.frame()])
                _launched(prof, FAST_FLOAT, c.name)
                check_float(c, outs[0], c.name)
        for We in (255, 2049):
            c = cat[col.width_name(64, We, 165, env32)]
            for dpt in (1, 2, 4, 8):
                outs, prof = ctx.render(c, [c.frame()], RR_OPT_FOV_DROPS_PER_THREAD=dpt)
                _launched(prof, FAST_FLOAT, c.name)
                check_float(c, outs[0], '%s dpt=%d' % (c.name, dpt))


@pytest.mark.parametrize('route', ['f64c', 'f64o'])
def test_widths_on_the_float64_routes(cat, route):
    with Ctx(next(iter(cat.values())).base) as ctx:
        for name in col.width_cases():
            c = cat[name]
            outs, prof = ctx.render(c, [c.frame()], route)
            _launched(prof, ('k_fov_spans', 'k_fov_sums'), name)
            assert 'k_fov_sort' not in prof, name
            check_f64(c, outs[0], '%s %s' % (name, route))
        for env32 in (True, False):
            for We in (255, 2049):
                c = cat[col.width_name(64, We, 165, env32)]
                for dpt in (1, 2, 4, 8):
                    outs, prof = ctx.render(c, [c.frame()], route, RR_OPT_FOV_DROPS_PER_THREAD=dpt)
                    check_f64(c, outs[0], '%s %s dpt=%d' % (c.name, route, dpt))


@pytest.mark.parametrize('He', col.HEIGHTS)
def test_heights(cat, He):
    """Padded span rows, empty bands, the three k_fov_spans instances as the list kernel (behind k_fov_dda) and as the every-drop
    kernel (RR_OPT_FOV_DDA 0, and the float64 route), the tallest map of the fast path; beyond it the general path, whose sums
    are float64 on either route."""
    c = cat['h%d' % He]
    fast = col.predict(c.He, c.We, (c.n,))['fast']
    with Ctx(c.base) as ctx:
        if fast:
            outs, prof = ctx.render(c, [c.frame()])
            _launched(prof, FAST_FLOAT, c.name)
            check_float(c, outs[0], c.name)
            outs, prof = ctx.render(c, [c.frame()], RR_OPT_FOV_DDA=0)
            _launched(prof, ('k_fov_spans', 'k_fov_sums'), c.name)
            assert 'k_fov_sort' not in prof and 'k_fov_vertices' not in prof, sorted(prof)
            check_float(c, outs[0], c.name + ' dda=0')
            for route in ('f64c', 'f64o'):
                outs, prof = ctx.render(c, [c.frame()], route)
                check_f64(c, outs[0], '%s %s' % (c.name, route))
        else:
            for cc in (c, cat['h1025_f64']):
                for route in ('f32', 'f64c'):
                    outs, prof = ctx.render(cc, [cc.frame()], route)
                    _launched(prof, ('k_fov_poly', 'k_fov_sums_general'), cc.name)
                    assert 'k_fov_sums' not in prof and 'k_fov_spans' not in prof, sorted(prof)
                    check_f64(cc, outs[0], '%s %s general' % (cc.name, route))


@pytest.mark.parametrize('dpt,n', col.DPT_CASES + ((0, col.BIG_N),))
def test_drops_per_thread_and_chunks(cat, dpt, n):
    """n = 1024 DPT - 1, 1024 DPT, 1024 DPT + 1 drops with the drops per thread forced, three chunks of 834 at one per thread, and the
    library's own choice for 8193 (two chunks of 4097 at eight per thread): the float route and the float64 one."""
    c = cat['big']
    with Ctx(c.base) as ctx:
        outs, prof = ctx.render(c, [c.frame(n)], RR_OPT_FOV_DROPS_PER_THREAD=dpt)
        _launched(prof, FAST_FLOAT, n)
        check_float(c, outs[0], 'big n=%d dpt=%d' % (n, dpt), n)
        outs, prof = ctx.render(c, [c.frame(n)], 'f64o', RR_OPT_FOV_DROPS_PER_THREAD=dpt)
        check_f64(c, outs[0], 'big n=%d dpt=%d f64o' % (n, dpt), n)
        outs, prof = ctx.render(c, [c.frame(n)], 'f64c', RR_OPT_FOV_DROPS_PER_THREAD=dpt)
        check_f64(c, outs[0], 'big n=%d dpt=%d f64c' % (n, dpt), n)


@pytest.mark.parametrize('dpt,n', [(1, 2500), (0, col.BIG_N)])
def test_order_walk_and_stream_give_the_same_bits(cat, dpt, n):
    """RR_OPT_FOV_ORDER 0 / 1 (k_fov_sort beyond one sweep of 1024, ties on both sides of a chunk boundary, list drops written
    through the inverse permutation into every chunk), RR_OPT_FOV_DDA 0 / 1 and RR_OPT_COLOUR_STREAM 0 / 1 on frames of several
    chunks: identical colour constants, and the table-order call against the reference too."""
    c = cat['big']
    with Ctx(c.base) as ctx:
        base, prof = ctx.render(c, [c.frame(n)], RR_OPT_FOV_DROPS_PER_THREAD=dpt)
        for opts in (dict(RR_OPT_FOV_ORDER=0), dict(RR_OPT_FOV_DDA=0), dict(RR_OPT_COLOUR_STREAM=0), dict(RR_OPT_FOV_ORDER=0, RR_OPT_COLOUR_STREAM=0)):
            outs, prof = ctx.render(c, [c.frame(n)], RR_OPT_FOV_DROPS_PER_THREAD=dpt, **opts)
            if 'RR_OPT_FOV_ORDER' in opts and len(opts) == 1:
                _launched(prof, FAST_FLOAT, opts)
                check_float(c, outs[0], 'big n=%d dpt=%d order=0' % (n, dpt), n)
            for k in ('colour', 'status'):
                differ = np.nonzero((outs[0][k] != base[0][k]).reshape(n, -1).any(axis=1))[0]
                assert not len(differ), (opts, k, len(differ), differ[:10])
        for first, count in col.BIG_TIES:                       # identical records: identical constants
            if first + count <= n:
                assert (base[0]['colour'][first:first + count] == base[0]['colour'][first]).all(), first


@pytest.mark.parametrize('dpt', [1, 0])
def test_a_batch_is_its_frames(cat, dpt):
    """Four frames of 0, 1, 1025 and 2500 drops under one capacity (the chunk size follows the frame, the drops per thread the
    batch; the frame stride of colpart / fband; an empty frame): every frame's constants are those of the frame alone, bit for
    bit, and within the bound of the reference."""
    c = cat['big']
    with Ctx(c.base) as ctx:
        frames = [c.frame(n) for n in col.BATCH_NS]
        outs, prof = ctx.render(c, frames, RR_OPT_FOV_DROPS_PER_THREAD=dpt)
        _launched(prof, FAST_FLOAT, dpt)
        for n, out in zip(col.BATCH_NS, outs):
            check_float(c, out, 'batch dpt=%d frame n=%d' % (dpt, n), n)
            alone, _ = ctx.render(c, [c.frame(n)], RR_OPT_FOV_DROPS_PER_THREAD=dpt)
            assert np.array_equal(alone[0]['colour'], out['colour']) and np.array_equal(alone[0]['status'], out['status']), (dpt, n)


def test_a_batch_of_mixed_image_types(cat):
    """The image as float64, float32 and bytes in one call: the colour branch never reads it."""
    for name in ('w64x255_c165_f32', 'w64x2049_c60_f64'):
        c = cat[name]
        with Ctx(c.base) as ctx:
            bg = c.base.bg
            frames = [c.frame(bg=b) for b in (bg, bg.astype(np.float32), np.round(bg * 255.0).astype(np.uint8))]
            outs, prof = ctx.render(c, frames)
            _launched(prof, FAST_FLOAT, name)
            for k, out in enumerate(outs):
                check_float(c, out, '%s image type %d' % (name, k))
                assert np.array_equal(out['colour'], outs[0]['colour']), (name, k)


@pytest.mark.parametrize('He,We', col.PLACEMENT_MAPS)
def test_polygon_placement_under_both_fill_rules(cat, He, We):
    """Spans ending in column 0 and in the last column, polygons on the first and the last row, inside one band and across every
    band boundary, across the seam, the 12-degree cone's narrow spans at the far right of the widest map, polygons of less
    than a row (a status): RR_OPT_FOV_FILL_RULE 1 and 0, the walk and the every-drop kernel."""
    with Ctx(next(iter(cat.values())).base) as ctx:
        for cone in col.CONES:
            c = cat['place%dx%d_c%d' % (He, We, cone)]
            for rule in (1, 0):
                outs, prof = ctx.render(c, [c.frame()], RR_OPT_FOV_FILL_RULE=rule)
                _launched(prof, FAST_FLOAT, c.name)
                check_float(c, outs[0], '%s rule=%d' % (c.name, rule), rule=rule)
                outs, prof = ctx.render(c, [c.frame()], RR_OPT_FOV_FILL_RULE=rule, RR_OPT_FOV_DDA=0)
                check_float(c, outs[0], '%s rule=%d dda=0' % (c.name, rule), rule=rule)
                outs, prof = ctx.render(c, [c.frame()], 'f64c', RR_OPT_FOV_FILL_RULE=rule)
                check_f64(c, outs[0], '%s rule=%d f64c' % (c.name, rule), rule=rule)
