"""GPU tier of the pre-pass pin (tests/prepass_cases.py): every case of the catalogue through RainHip.prepass_frames against the
float64 reference within the counted bounds, a batch that mixes element types and fog constants, size and tap-count changes
on a live context, and the map-only mode from a float32 and a uint8 image.  No frame is larger than 192 x 32 or 72 x 257."""
import numpy as np
import pytest

import helpers as h
import prepass_cases as pc
from oracle import prepass as op

pytestmark = pytest.mark.gpu


def _geometry(rh, H, W):
    return rh.set_envmap_geometry(H, W, *pc.envmod.EnvironmentMapGenerator(pc.FOCAL, W, H).device_tables(H, W))


def _taps(rh, taps):
    rh.set_prepass_kernels(pc.fog_taps(taps[0]), pc.env_taps(taps[1]))


def _run(rh, frames, want_env=True, out_dtype=np.float64):
    return rh.prepass_frames(frames, want_env=want_env, want_env_u8=want_env, out_dtype=out_dtype)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("H,W", pc.sizes(), ids=['%dx%d' % s for s in pc.sizes()])
def test_catalogue_on_the_device(built, H, W):
    """One context per size; a case sets its own tap counts.  Both output widths: the float32 arrays are the float64 ones rounded
    once, bit for bit."""
    cases = pc.cases_of(H, W)
    for c in cases:
        c.assert_reaches_clamps()                      # from the reference alone, before the device is asked
    rh = h.hb.RainHip(0)
    _taps(rh, cases[0].taps)
    We = _geometry(rh, H, W) if cases[0].want_env else 0
    for c in cases:
        _taps(rh, c.taps)
        o = _run(rh, [c.frame()], c.want_env)[0]
        n = _run(rh, [c.frame()], c.want_env, np.float32)[0]
        d = c.check_fog(o['rainy_bg'], n['rainy_bg'])
        print('%s: max |d| %.3g, bound %.3g' % (c.name, d, c.bound))
        if c.want_env:
            assert o['env_bgr_u8'].shape == (H, We, 3)
            c.check_map(o['rainy_bg'], o['env_bgr_u8'], o['env_xyY'], n['env_xyY'], n['env_bgr_u8'])
    rh.close()


def test_mixed_batch(built):
    """Five frames of one call with three depth types, three image types, both kinds of input and five rain intensities: the
    per-frame type bits, fog constants and `f * px` / `f * 3 + c` offsets.  Each frame is its own single-frame call, bit for bit,
    and within its bound of the reference."""
    H, W = 65, 33
    kinds = [('scene', np.float64, np.float32, 10), ('sat', np.float32, np.float64, 200), ('scene', np.uint8, np.uint16, 25),
             ('sat', np.uint8, np.float32, 100), ('scene', np.float32, np.float64, 50)]

    def make(taps):
        out = []
        for kind, it, dt, rain in kinds:
            c = pc.Case(H, W, kind, it, dt, taps)
            c.rain = rain                              # (before anything is computed from it)
            out.append(c)
        return out

    cases = make((25, 15))
    assert len({c.rain for c in cases}) == 5 and len({float(c.parts['k3'][0]) for c in cases}) == 5       # five beta_ext, five means
    rh = h.hb.RainHip(0)
    _taps(rh, (25, 15))
    _geometry(rh, H, W)
    singles = [_run(rh, [c.frame()])[0] for c in cases]
    batch = _run(rh, [c.frame() for c in cases])
    batch32 = _run(rh, [c.frame() for c in cases], out_dtype=np.float32)
    for c, s, b, n in zip(cases, singles, batch, batch32):
        _same(s, b, c.name)
        c.check_fog(b['rainy_bg'], n['rainy_bg'])
        c.check_map(b['rainy_bg'], b['env_bgr_u8'], b['env_xyY'], n['env_xyY'], n['env_bgr_u8'])
    # the three-kernel form has its own per-frame planes
    cases = make((9, 15))
    _taps(rh, (9, 15))
    singles = [_run(rh, [c.frame()])[0] for c in cases]
    batch = _run(rh, [c.frame() for c in cases])
    for c, s, b in zip(cases, singles, batch):
        _same(s, b, c.name)
        c.check_fog(b['rainy_bg'])
        c.check_map(b['rainy_bg'], b['env_bgr_u8'], b['env_xyY'])
    rh.close()


def test_live_context_follows_size_and_tap_changes(built):
    """enqueue_prepass re-allocates its scratch on H != pre_H, planes && !pre_planes and We > pre_We, and rebuilds d_need_h when
    the map's tap count changes: every step on ONE context equals a fresh context's result, bit for bit."""
    big, small = (136, 40), (9, 5)
    cb = [pc.Case(*big, kind, np.float64, dt) for kind, dt in (('scene', np.float32), ('sat', np.float64), ('scene', np.uint16))]
    cs = [pc.Case(*small, 'sat', np.float64, np.float32)]
    steps = [(big, (25, 15), cb[:1], False),    # the fog layer alone: scratch without a map (pre_We = 0)
             (big, (25, 15), cb[:1], True),     # We > pre_We; k_fog_tile, two segments of 72 and 64 rows
             (big, (9, 15), cb[:1], True),      # the planes are allocated late
             (big, (25, 33), cb[1:2], True),    # need_h for 33 taps ...
             (big, (25, 15), cb[1:2], True),    # ... and for 15 again, the same geometry
             (small, (25, 15), cs, True),       # another size: after set_envmap_geometry
             (big, (25, 15), cb[:1], True),     # and back
             (big, (25, 15), cb, True),         # a batch of 3 after batches of 1
             (big, (3, 1), cb, True)]           # ... and its planes
    live = h.hb.RainHip(0)
    size = None
    for i, (sz, taps, cases, env) in enumerate(steps):
        frames = [c.frame() for c in cases]
        _taps(live, taps)
        if sz != size:
            _geometry(live, *sz)
            size = sz
        got = _run(live, frames, env)
        fresh = h.hb.RainHip(0)
        _taps(fresh, taps)
        _geometry(fresh, *sz)
        want = _run(fresh, frames, env)
        fresh.close()
        for g, w in zip(got, want):
            _same(g, w, ('step', i))
        # and the fresh context's result is the reference's map of its own fog layer (a wrong need_h shows here)
        for c, w in zip(cases, want if env else []):
            assert np.array_equal(w['env_bgr_u8'], pc.map_bytes(pc.ref_env_map(w['rainy_bg'], pc.env_taps(taps[1])))), ('step', i, c.name)
    live.close()


def _env_only(rh, image, in_types, want_xyY=True):
    """rr_prepass_frames in the map-only mode, the structs filled as test_gpu_prepass.test_reference_signature_seams does."""
    H, W = image.shape[:2]
    We = rh._check(rh.lib.rr_envmap_width(rh.h), 'rr_envmap_width')
    pin = (h.hb.rr_prepass_in * 1)()
    pout = (h.hb.rr_prepass_out * 1)()
    keep = np.ascontiguousarray(image)
    u8 = np.zeros((H, We, 3), np.uint8)
    xyY = np.full((H, We, 3), np.nan)
    pin[0].H, pin[0].W, pin[0].bg, pin[0].mode, pin[0].in_types = H, W, keep.ctypes.data, h.hb.RR_PRE_ENV_ONLY, in_types
    pout[0].env_bgr_u8, pout[0].env_xyY = u8.ctypes.data, xyY.ctypes.data
    rh._check(rh.lib.rr_prepass_frames(rh.h, 1, pin, pout), 'rr_prepass_frames')
    return u8, xyY


@pytest.mark.parametrize("H,W", [(13, 33), (72, 257)])
def test_map_only_mode_reads_every_image_type(built, H, W):
    """RR_PRE_ENV_ONLY reads `bg` through bg8_px / load_unit: a float32 and a uint8 image (in_types) give the map of the float64
    image holding the same values -- the suite's scene and the saturating one, whose black cells give xyY = 0, not nan."""
    rh = h.hb.RainHip(0)
    _taps(rh, (25, 15))
    _geometry(rh, H, W)
    for kind in ('scene', 'sat'):
        img = pc.Case(H, W, kind, np.float64, np.float64).inputs[0]
        for narrow, bits in ((img.astype(np.float32), h.hb.RR_IN_BG_F32), ((img * 255).astype(np.uint8), h.hb.RR_IN_BG_U8)):
            wide = pc.widen(narrow)
            e_bgr = op.generate_env_map(wide, pc.FOCAL)
            want8 = pc.map_bytes(e_bgr)
            if kind == 'sat':
                assert (want8 == 0).all(axis=-1).any()
            a8, axyY = _env_only(rh, narrow, bits)
            b8, bxyY = _env_only(rh, wide, 0)
            assert np.array_equal(a8, b8) and np.array_equal(axyY, bxyY), (kind, narrow.dtype)
            assert np.array_equal(a8, want8), (kind, narrow.dtype)
            assert not np.isnan(axyY).any()
            assert np.abs(axyY - op.env_to_xyY(e_bgr)).max() < pc.XYY_TOL
            if kind == 'sat':
                assert (axyY[(want8 == 0).all(axis=-1)] == 0.0).all()
    rh.close()
