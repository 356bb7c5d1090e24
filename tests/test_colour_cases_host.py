"""CPU tier: the colour catalogue (tests/colour_cases.py) put on trial before the GPU tier relies on it.  The reference equals
the oracle's own polygon and literal mask fill on a sample of every case; the catalogue reaches every template instance and
every feature it names (a host-side predictor of the launch code says which); the rounding bound holds for a float32
restatement of the row scan's structure on every case, and every mistake the catalogue is aimed at leaves it."""
import ctypes
import re

import numpy as np
import pytest

import colour_cases as col
import helpers as h
from oracle import cvlike
from oracle import render as orc


@pytest.fixture(scope='module')
def cat(tmp_path_factory):
    base = col.Base(lambda n: tmp_path_factory.mktemp(n))
    return col.build(base)


def _chunk_edges(n):
    out = set()
    for dpt, m in col.DPT_CASES + ((0, col.BIG_N),) + tuple((1, k) for k in col.BATCH_NS):
        if 0 < m <= n:
            p = col.predict(64, 255, (m,), dpt=dpt)
            for c in range(1, p['nchunk']):
                out |= {c * p['per'][0] - 1, c * p['per'][0]}
    return sorted(i for i in out if 0 <= i < n)


def _sample(c, limit=40):
    """first, last, both sides of every chunk boundary, wrapping drops, the extreme placements -- at most `limit`."""
    if c.n == 0:
        return []
    f = c.features()
    pick = [0, c.n - 1]
    if 'chunks' in c.aims:
        pick += _chunk_edges(c.n)
    for k in ('col0', 'col_last', 'row0', 'row_last', 'one_band', 'narrow', 'far_right', 'seam', 'wrap'):
        pick += list(np.nonzero(f[k])[0][:2])
    pick += list(np.nonzero(f['wrap'])[0][2:8])
    rng = np.random.RandomState(c.n + c.We)
    pick += list(rng.permutation(c.n)[:limit])
    out = []
    for i in pick:
        if int(i) not in out:
            out.append(int(i))
    return out[:limit]


def test_reference_equals_the_oracle(cat):
    """compute_fov_plane_points + the literal mask fill + bad_weather.py's chain against reference_sums / reference_K: 1e-12."""
    checked = 0
    for name, c in cat.items():
        # (the literal fill is a Python loop per texel row: fewer drops on the maps of 10^5 texels)
        limit = 40 if c.He * c.We <= 20000 else 20
        fc = orc.FrameConsts(c.map.env, c.map.omega)
        assert abs(fc.sum_omega - c.map.sumW) <= 1e-12 * c.map.sumW
        for rule, rname in ((1, 'cv'), (0, 'span')):
            if rule == 0 and 'placement' not in c.aims:
                continue
            r = c.ref(rule)
            cvlike.set_fill_rule(rname, int(c.cam.n_fov))
            try:
                for i in _sample(c, limit):
                    d = c.drops[i]
                    pts = orc.compute_fov_plane_points(d['wps'].copy(), d['wpe'].copy(), orc.RADIUS, c.cone, orc.N_FOV, (c.He, c.We))
                    ok = len(pts) > 0 and np.all(np.isfinite(pts)) and not cvlike.polygon_all_collinear(cvlike.polygon_to_int(pts))
                    o = orc.fov_colour(c.map.env, c.map.omega, cvlike.polygon_to_int(pts), fc, faithful=True) if ok else None
                    if o is None:
                        assert r['status'][i] in (orc.ST_FOV_FAIL, orc.ST_EMPTY_FOV) and not r['K'][i].any(), (name, i)
                        continue
                    assert r['status'][i] == 0, (name, i)
                    xy, drop_Y = o
                    want = np.array([xy[0], xy[1], col.GRAY_Y * drop_Y])
                    assert np.abs(r['xyY'][i] - want).max() <= 1e-12 * np.abs(want).max(), (name, rname, i, r['xyY'][i], want)
                    K = orc.convert_xyY_to_rgb(want)[::-1]
                    assert np.abs(r['K'][i] - K).max() <= 1e-12 * np.abs(K).max(), (name, rname, i)
                    assert np.abs(col.unmix(r['K'][i]) - want).max() <= 1e-12 * np.abs(want).max(), (name, i)
                    checked += 1
            finally:
                cvlike.set_fill_rule()
    assert checked > 800


def test_reference_statuses_equal_the_host_build(cat):
    """The statuses and constants the GPU tier compares with, against the host build's whole-frame render (1e-9, the bar the
    suite holds the float64 kernels to)."""
    for name in ('w64x21_c60_f32', 'h20', 'h1025', 'place16x4096_c12', 'place64x255_c12', 'place64x255_c165'):
        c = cat[name]
        for rule in ((1, 0) if 'placement' in c.aims else (1,)):
            status, K = c.emu_status(rule)
            r = c.ref(rule)
            assert np.array_equal(status, r['status']), name
            assert np.abs(K - r['K']).max() <= 1e-9 * np.abs(r['K']).max(), name


def test_catalogue_reaches_what_it_names(cat):
    seen, emax = set(), set()
    for name, ns, kw in col.runs():
        c = cat[name]
        p = col.predict(c.He, c.We, ns, dpt=kw.get('dpt', 0), route=kw['route'], env32=c.env32, dda=kw.get('dda', 1))
        assert kw.get('env32', True) == c.env32, name
        seen |= p['instances']
        if p['fast']:
            emax.add(p['emax'])
    sums32 = {'k_fov_sums32<%d, %d, %s>' % (d, e, t) for d in (1, 2, 4, 8) for e in (1, 2) for t in ('true', 'false')}
    sums64 = {'k_fov_sums<%d, %d>' % (d, e) for d in (1, 2, 4, 8) for e in (1, 2)}
    spans = {'k_fov_spans<%d, %s>' % (k, r) for k in (6, 8, 16) for r in ('true', 'false')}
    assert len(sums32) == 16 and len(sums64) == 8 and len(spans) == 6
    assert seen == sums32 | sums64 | spans | {'k_fov_poly_general', 'k_fov_sums_general'}, (sums32 | sums64 | spans) ^ seen
    assert emax == {1, 2}
    # every instance the dispatch names is one of those (a new one must come with a case)
    src = col._hip_source()
    assert {m.replace(' ', '') for m in re.findall(r'k_fov_sums32<\d, \d, \w+>', src)} == {s.replace(' ', '') for s in sums32}
    assert {m.replace(' ', '') for m in re.findall(r'\(k_fov_sums<\d, \d>\)', src)} == {'(%s)' % s.replace(' ', '') for s in sums64}
    assert {m.replace(' ', '') for m in re.findall(r'k_fov_spans<\d+, \w+>', src)} >= {s.replace(' ', '') for s in spans}
    # widths
    p = col.predict(64, 20, (col.N_SMALL,))
    assert p['idle_waves'] == list(range(10, 16)) and p['Cw'] == 2
    assert col.predict(64, 2048, (1,))['emax'] == 1 and col.predict(64, 2049, (1,))['emax'] == 2 and col.predict(16, 4096, (1,))['fast']
    for He, We in col.WIDTHS:
        for cone in (165, 60):
            f = cat[col.width_name(He, We, cone, True)].features()
            assert f['col0'].sum() >= 8 and f['col_last'].sum() >= 8 and f['wrap'].sum() >= 8, (He, We, cone)
    # heights: rpb, empty bands, padded rows; the three k_fov_spans classes; the general path
    p = col.predict(20, col.HEIGHTS_WE, (col.N_SMALL,))
    assert p['rpb'] == 4 and p['empty_bands'] == [5, 6, 7] and p['Hp'] == 20
    assert col.predict(63, 96, (1,))['Hp'] == 64 and col.predict(513, 96, (1,))['Hp'] == 516
    assert [col.predict(He, 96, (1,))['spans'] for He in (384, 385, 512, 513)] == ['k_fov_spans<6, true>', 'k_fov_spans<8, true>',
                                                                                 'k_fov_spans<8, true>', 'k_fov_spans<16, true>']
    assert col.predict(1024, 96, (1,))['fast'] and not col.predict(1025, 96, (1,))['fast']
    for He in col.HEIGHTS:
        f = cat['h%d' % He].features()
        assert f['row0'].sum() >= 4 and f['row_last'].sum() >= 4 and f['wrap'].sum() >= 8, He
    # chunks
    big = cat['big']
    for dpt, n in col.DPT_CASES:
        p = col.predict(64, 255, (n,), dpt=dpt)
        assert p['DPT'] == dpt and p['nchunk'] == -(-n // (1024 * dpt)), (dpt, n)
    assert col.predict(64, 255, (2500,), dpt=1)['nchunk'] == 3 and col.predict(64, 255, (2500,), dpt=1)['per'] == [834]
    p = col.predict(64, 255, (col.BIG_N,))
    assert p['DPT'] == 8 and p['nchunk'] == 2 and p['per'] == [4097]
    p = col.predict(64, 255, col.BATCH_NS, dpt=1)
    assert p['nchunk'] == 3 and p['per'] == [0, 1, 342, 834]
    assert col.BIG_N > 3 * 64 * col.FOV_SORT_WAVES                     # k_fov_sort: more than one sweep of 1024 per pass, per wave
    f = big.features()
    wrap = np.nonzero(f['wrap'])[0]
    for n, per in ((2500, 834), (col.BIG_N, 4097), (1025, 513), (2049, 1025)):      # a 24-gon in every chunk, on both sides of every boundary's neighbourhood
        for c0 in range(0, n, per):
            assert ((wrap >= c0) & (wrap < min(n, c0 + per))).any(), (n, c0)
    assert f['wrap'][0]                                                  # the one-drop frame's drop takes the list
    for first, count in col.BIG_TIES:
        assert all(big.drops[first + k].tobytes() == big.drops[first].tobytes() for k in range(count))
    for edge in (834, 1668, 4097):                                       # equal records on both sides of a chunk boundary (table order)
        assert any(first < edge < first + count for first, count in col.BIG_TIES), edge
    # placement
    for He, We in col.PLACEMENT_MAPS:
        got = {}
        for cone in col.CONES:
            c = cat['place%dx%d_c%d' % (He, We, cone)]
            for rule in (1, 0):
                for k, v in c.features(rule).items():
                    got[k] = got.get(k, 0) + int((v & c.ref(rule)['composited']).sum())
        r = col.Map.get(He, We, True).rpb()
        need = ['col0', 'col_last', 'row0', 'row_last', 'one_band', 'seam', 'wrap', 'far_right'] + ['straddle_%d' % b for b in range(1, 8) if b * r < He]
        assert all(got.get(k, 0) >= 4 for k in need), (He, We, {k: got.get(k, 0) for k in need if got.get(k, 0) < 4})
    f = cat['place16x4096_c12'].features()
    xl, xr = cat['place16x4096_c12'].spans()
    wide = (xr - xl + 1).max(axis=1)
    assert (f['far_right'] & (wide < 4096 // 16) & (wide > 0)).sum() >= 3   # the 12-degree cone's spans, 3 % of the width, in the last sixteenth
    assert (cat['place16x4096_c12'].ref()['status'] == orc.ST_FOV_FAIL).sum() >= 10      # polygons of less than a row: a status, K = 0


def _left(case_ref, xyY):
    """drops whose (x, y, Yg) lie outside the bound around the reference (a NaN -- no texel left -- is outside)"""
    return ~(np.abs(xyY - case_ref['xyY']) <= case_ref['bound']).all(axis=1)


def test_bound_is_sound_for_a_float32_scan(cat):
    """k_fov_sums32's structure in numpy float32 (colour_cases.float_prefix / float_sums) stays inside rounding_bound on every
    case, drop and component; and is no bit-exact copy: it is float, it does differ from the reference."""
    worst = {}
    for name, c in cat.items():
        if not col.predict(c.He, c.We, (c.n,))['fast']:
            continue
        for rule in ((1, 0) if 'placement' in c.aims else (1,)):
            r = c.ref(rule)
            xl, xr = c.spans(rule)
            S, sw, sy = col.float_sums(c.map, xl, xr)
            got = col.xyY_of_sums(S, sw, sy)
            comp = r['composited']
            ratio = np.abs(got - r['xyY'])[comp] / r['bound'][comp]
            assert (ratio <= 1.0).all(), (name, rule, ratio.max())
            assert ratio.max() > 1e-4, name
            worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
    assert len(worst) >= 50 and max(worst.values()) <= 1.0


# what a mistake does to the reference's sums: (name, function(case, rule, n, per) -> (S', touched drops))
def _mut_spans(dl, dr):
    def f(c, rule, n, per):
        xl, xr = c.spans(rule)
        xl, xr = xl[:n] + dl, xr[:n] + dr
        return col.span_sums(c.map.P, xl, xr), (c.spans(rule)[0][:n] <= c.spans(rule)[1][:n]).any(1)
    return f


def _mut_band_row(c, rule, n, per):
    xl, xr = c.spans(rule)
    xl, xr = xl[:n].copy(), xr[:n].copy()
    r = c.map.rpb()
    last = [min(c.He, (b + 1) * r) - 1 for b in range(col.COL_PARTS) if b * r < c.He]
    touched = (xl[:, last] <= xr[:, last]).any(1)
    xl[:, last], xr[:, last] = 1, 0
    return col.span_sums(c.map.P, xl, xr), touched


def _mut_last_column(c, rule, n, per):
    env = c.map.env.copy()
    om = c.map.omega.copy()
    om[:, -1] = 0.0
    xl, xr = c.spans(rule)
    return col.span_sums(col.Map.prefix(env, om), xl[:n], xr[:n]), ((xl[:n] <= xr[:n]) & (xr[:n] + 1 == c.We)).any(1)


def _mut_next_column(c, rule, n, per):
    S = c.ref(rule)['S'][:n]
    out = np.roll(S, -1, axis=0)
    out[-1] = S[-1]
    return out, np.arange(n) < n - 1


def _mut_first_chunk(c, rule, n, per):
    S = c.ref(rule)['S'][:n].copy()
    i = np.arange(n)
    S[per:] = S[i[per:] % per]
    return S, i >= per


def _mut_index_for_slot(c, rule, n, per):
    S = c.ref(rule)['S'][:n]
    order = col.surrogate_order(c, n, rule)
    out, touched = S.copy(), np.zeros(n, bool)
    for i in np.nonzero(c.features(rule)['wrap'][:n])[0]:
        j = order[i]                                   # the drop whose slot is i reads what the 24-gon left at its INDEX
        if j != i:
            out[j], touched[j] = S[i], True
    return out, touched


MISTAKES = (('xr+1 -> xr', _mut_spans(0, -1), None), ('xl -> xl+1', _mut_spans(1, 0), None), ("a band's last row skipped", _mut_band_row, None),
            ('last column of an odd width dropped', _mut_last_column, 'odd_width'), ('drop i reads column i+1', _mut_next_column, None),
            ("the second chunk reads the first chunk's columns", _mut_first_chunk, 'chunks'),
            ("a 24-gon's sums at its index, not its slot", _mut_index_for_slot, 'order'))


def test_bound_is_sharp_enough_for_the_mistakes_aimed_at(cat):
    """Each mistake, applied to the float64 reference, leaves rounding_bound for at least 90 % of the drops it touches, in every
    case that aims at it."""
    for name, c in cat.items():
        if not col.predict(c.He, c.We, (max(c.n, 1),))['fast']:
            continue                                   # the general path is held to 1e-9
        for label, fn, aim in MISTAKES:
            if aim is not None and aim not in c.aims:
                continue
            sizes = ((2500, 834), (col.BIG_N, 4097), (1025, 513), (2049, 1025)) if aim in ('chunks', 'order') else ((c.n, c.n),)
            for rule in ((1, 0) if 'placement' in c.aims else (1,)):
                r = c.ref(rule)
                for n, per in sizes:
                    S, touched = fn(c, rule, n, per)
                    sub = dict(xyY=r['xyY'][:n], bound=r['bound'][:n])
                    touched = touched & r['composited'][:n]
                    left = _left(sub, col.xyY_of_sums(S, c.map.sumW, c.map.sumY))
                    assert touched.sum() >= 4, (name, label, int(touched.sum()))
                    share = (left & touched).sum() / touched.sum()
                    assert share >= 0.9, (name, label, rule, n, share, int(touched.sum()))
                    assert not (left & ~touched & r['composited'][:n]).any(), (name, label)


def test_host_float_polygon_rarely_differs(cat):
    """The share of drops whose host float polygon (fov_polygon_auto, used32 = 1) differs from the float64 one: under 0.5 % in
    every case -- the condition under the GPU tier's cap on exception drops."""
    emu = h.hostemu()
    for name, c in cat.items():
        n = c.n
        p32, n32, used = np.zeros(n * 72, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        d = np.ascontiguousarray(c.drops)
        emu.emu_fov_auto(h._p(d), n, ctypes.byref(c.cam), c.He, c.We, h._p(p32), h._p(n32), h._p(used))
        poly, npts, _plans, _sizes = c.polygons()
        assert np.array_equal(n32, npts), name
        differs = (used == 1) & (p32.reshape(n, 2, 36) != poly).any(axis=(1, 2))
        assert differs.sum() < 0.005 * n, (name, int(differs.sum()), n)
