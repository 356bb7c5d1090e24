"""GPU tier of the rain layer (csrc/rr_layer.h k_rain_layer): the compositor catalogues through the C ABI against the
float64 reference of tests/rain_layer.py at its derived bound, and what arming must not touch -- the image, the mask, the statuses,
the other slots, the unarmed launches.  Then RainAugment(return_layer=True)."""
import ctypes
import importlib
import types

import numpy as np
import pytest
import torch

import compositor_cases as cc
import helpers as h
import rain_layer as rl
import test_gpu_augment as tga
import test_gpu_compositor_cases as tcc

pytestmark = pytest.mark.gpu

hb = h.hb
augment = tga.augment
DEV = tga.DEV
NAMES = ('seams_low', 'seams_high', 'lengths', 'indices', 'tiles_1', 'tiles_3', 'tiles_7', 'tiles_8', 'tiles_9', 'wide', 'segment_dim')
F64 = dict(RR_OPT_FOV_F32=0)                    # float64 colour constants: the float colour branch's own error is tests/colour_cases.py's
RR_E_ARG, RR_E_STATE = -1, -4


class Catalogue:
    """name -> Case; references (rl.reference) made once per (case, depth) and never changed."""

    def __init__(self, mk):
        tpl = cc.Templates(mk('tpl'))
        cases = [cc.seams(mk('sl'), tpl, 'low'), cc.seams(mk('sh'), tpl, 'high'), cc.lengths(mk('le'), tpl), cc.indices(mk('in'), tpl),
                 rl.segment_dim(mk('sd'), tpl)] + cc.shapes(mk, tpl)
        self.cases = {c.name: c for c in cases}
        self.refs = {}

    def __getitem__(self, name):
        return self.cases[name]

    def ref(self, name, depth=None):
        key = (name, depth is not None)
        if key not in self.refs:
            self.refs[key] = rl.reference(self.cases[name], depth=depth)
        return self.refs[key]


@pytest.fixture(scope='module')
def cat(built, tmp_path_factory):
    return Catalogue(lambda n: tmp_path_factory.mktemp(n))


def _render(c, frames, want_layer=True, want_composite=False, **opts):
    rh = tcc._ctx(c, **opts)
    try:
        return rh.render_frames(frames, want_composite=want_composite, want_layer=want_layer)
    finally:
        rh.close()


def _same_outputs(a, b, what):
    for k in ('image_u8', 'mask', 'mask_i32', 'status'):
        assert np.array_equal(a[k], b[k]), '%s: %s differs' % (what, k)


def _within_bound(c, out, ref, what):
    L, T = out['layer'][..., :3].astype(np.float64), out['layer'][..., 3].astype(np.float64)
    bnd = rl.bound(ref)
    eL, eT = np.abs(L - ref['L']).max(axis=2), np.abs(T - ref['T'])
    print('%s %s: max |dL| %.3g, max |dT| %.3g, largest share of the bound %.3f (max n %d)' % (
        c.name, what, eL.max(), eT.max(), max((eL / bnd).max(), (eT / bnd).max()), ref['n'].max()))
    for key, e in (('L', eL), ('T', eT)):
        bad = e > bnd
        assert not bad.any(), '%s %s: %s misses the bound by up to %.3g: %s' % (c.name, what, key, (e - bnd).max(), cc.where(c, bad, cc.GEOM32))
    dry = ref['n'] == 0
    assert (out['layer'][dry][:, 3] == 1).all() and (out['layer'][dry][:, :3] == 0).all(), '%s %s: a pixel no drop lists' % (c.name, what)
    assert np.array_equal(out['status'], ref['status'])


# ---- 1. every catalogue against the reference; arming leaves the other outputs alone ---------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_catalogue_layer_matches_reference(cat, name):
    c = cat[name]
    armed = _render(c, [c.frame()], True, **F64)[0]
    plain = _render(c, [c.frame()], False, **F64)[0]
    assert armed['layer'].dtype == np.float32 and armed['layer'].shape == (c.H, c.W, 4) and 'layer' not in plain
    _within_bound(c, armed, cat.ref(name), 'armed')
    _same_outputs(armed, plain, name + ': armed vs unarmed')
    assert armed['layer'][..., 3].min() < 1 and armed['layer'][..., :3].max() > 0


# ---- 2. recomposition: the layer over the frame's own image is the frame's rainy image ----------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_layer_over_the_background_is_the_rainy_image(cat, name):
    """Default options.  The catalogue frames do not clamp (their own float64 composite peaks at 0.8), so the composite is
    T bg + L; the 1 LSB is the image contract's: the truncation to bytes turns the float chain's 1e-4 into at most one code."""
    c = cat[name]
    out = _render(c, [c.frame()])[0]
    lay = out['layer'].astype(np.float64)
    v = np.clip(lay[..., 3:4] * c.bg + lay[..., :3] - out['shift'], 0.0, 1.0)
    rgb = (v * 255.0).astype(np.uint8)[..., ::-1]                        # B G R -> R G B
    d = np.abs(rgb.astype(int) - out['image_u8'].astype(int))
    print('%s: shift %.6g, max |d| %d LSB, %d px differ' % (name, out['shift'], d.max(), (d > 0).any(axis=2).sum()))
    assert d.max() <= 1, cc.where(c, (d > 1).any(axis=2), cc.GEOM32)
    assert (out['mask'] > 0).any()


# ---- 3. the layer does not depend on which compositor made the image ----------------------------------------------------------------
@pytest.mark.parametrize('name', ['seams_low', 'lengths'])
def test_layer_bits_across_the_compositor_configurations(cat, name):
    c = cat[name]
    outs = {}
    for config, (opts, want, _geom) in tcc.CONFIGS.items():
        outs[config] = _render(c, [c.frame()], True, want, **dict(opts, **F64))[0]
    for config, o in outs.items():
        assert np.array_equal(o['layer'].view(np.uint32), outs['default']['layer'].view(np.uint32)), config
        print('%s %s: shift %.12g' % (name, config, o['shift']))
    comp = outs['composite']                                             # the float64 composite is asked for: k_finalize's diff
    want = comp['rainy_bg'].mean() - c.bg.mean()
    assert abs(comp['shift'] - want) <= 1e-6, (comp['shift'], want)
    assert abs(comp['shift']) > 1e-6


# ---- 4. ... nor on the image -----------------------------------------------------------------------------------------------------------
def test_layer_bits_do_not_depend_on_the_image(cat):
    c = cat['seams_low']
    base = _render(c, [c.frame()])[0]
    for bg in (np.round(c.bg * 255).astype(np.uint8), c.bg.astype(np.float32)):
        o = _render(c, [c.frame(bg=bg)])[0]
        assert np.array_equal(o['layer'].view(np.uint32), base['layer'].view(np.uint32)), bg.dtype
        assert np.array_equal(o['mask'], base['mask'])


# ---- 5. depth occlusion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seams_high', 'lengths'])
def test_depth_wall_hides_drops_from_the_layer(cat, name):
    c = cat[name]
    wall = tcc._wall(c)
    ref = cat.ref(name, depth=wall)
    assert (ref['T'] != cat.ref(name)['T']).any()
    out = _render(c, [c.frame(depth=wall)], True, RR_OPT_DEPTH_OCCLUSION=1, **F64)[0]
    _within_bound(c, out, ref, 'behind the wall')


# ---- 6. batches ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['default', 'composite'])
def batch(cat, request):
    """(config, the three frames alone, the three frames in one call) under the float compositor and under the float64 one."""
    c = cat['seams_low']
    want = request.param == 'composite'
    tables = [c.drops, c.drops[::2], np.zeros(0, hb.DROP_DTYPE)]
    rh = tcc._ctx(c)
    try:
        alone = [rh.render_frames([c.frame(t)], want_composite=want, want_layer=True)[0] for t in tables]
        together = rh.render_frames([c.frame(t) for t in tables], want_composite=want, want_layer=True)
    finally:
        rh.close()
    return request.param, alone, together


def test_batch_frames_equal_their_single_calls(batch):
    _config, alone, together = batch
    for f, (a, t) in enumerate(zip(alone, together)):
        assert np.array_equal(a['layer'].view(np.uint32), t['layer'].view(np.uint32)), f
        assert a['shift'] == t['shift'], f
        _same_outputs(a, t, 'frame %d' % f)
    assert not np.array_equal(together[0]['layer'], together[1]['layer'])
    assert (together[2]['layer'][..., 3] == 1).all() and (together[2]['layer'][..., :3] == 0).all()


def test_empty_frame_has_no_shift(batch):
    """shift is the diff the finalize kernels subtract, means[4 f] - means[4 f + 1] = mean(composite) - mean(bg).  A frame without
    drops has composite == bg, so the diff is 0 -- exactly so where the compositor holds the image exactly: the float64
    compositor of the 'composite' batch sums the same values twice, and shift == 0 is asserted as it stands.  k_composite32 (the
    'default' batch) carries the catalogue's float64 image in float32: its composite is float(bg), every value of [0, 1] off by
    at most 2^-25 (half an ulp below 1), so is the mean of those errors; the two float64 sums of 3 H W values in [0, 1] add at
    most 3 H W 2^-53 each to a mean.  Measured there: 1.8e-11.  (For a float32 image k_composite32 holds it exactly too:
    test_empty_frame_shift_is_zero_for_a_float32_image.)"""
    config, _alone, together = batch
    shift = together[2]['shift']
    print('%s: shift of the frame without drops: %.17g' % (config, shift))
    if config == 'composite':
        assert shift == 0
    else:
        H, W = together[2]['layer'].shape[:2]
        assert abs(shift) <= 2.0 ** -25 + 2 * 3 * H * W * 2.0 ** -53


def test_empty_frame_shift_is_zero_for_a_float32_image(cat):
    """The float compositor on an image it holds exactly: composite == bg, value for value, the two means are the same sums."""
    c = cat['seams_low']
    out = _render(c, [c.frame(np.zeros(0, hb.DROP_DTYPE), bg=c.bg.astype(np.float32))])[0]
    assert out['shift'] == 0 and (out['layer'][..., 3] == 1).all()


# ---- 7. the asynchronous route ---------------------------------------------------------------------------------------------------------
def _outs(rh, c):
    return dict(image_u8=rh.host_array((c.H, c.W, 3), np.uint8), mask=rh.host_array((c.H, c.W), np.float64),
                mask_i32=rh.host_array((c.H, c.W), np.int32), status=np.zeros(len(c.drops), np.int32))


def _run(rh, slot, c, o):
    rh.pipeline_submit(slot, [c.frame()], [o])


def test_armed_slot_beside_an_unarmed_one(cat):
    s, le = cat['seams_low'], cat['lengths']
    rh = tcc._ctx(s)
    try:
        want_s = rh.render_frames([s.frame()], want_composite=False, want_layer=True)[0]
        want_l = rh.render_frames([le.frame()], want_composite=False)[0]
        lay = dict(layer=rh.host_array((s.H, s.W, 4), np.float32), shift=rh.host_array((1,), np.float64))
        o_s, o_l = _outs(rh, s), _outs(rh, le)
        rh.pipeline_set_layer(1, [lay])
        for _round in range(2):
            lay['layer'][...] = -7.0
            lay['shift'][0] = -7.0
            _run(rh, 0, le, o_l)
            _run(rh, 1, s, o_s)
            while not rh.pipeline_wait(1):               # (RR_E_ARENA: the re-submit applies the armed state once more)
                _run(rh, 1, s, o_s)
            assert np.array_equal(lay['layer'].view(np.uint32), want_s['layer'].view(np.uint32)) and lay['shift'][0] == want_s['shift']
            _same_outputs(o_s, want_s, 'slot 1')
            while not rh.pipeline_wait(0):
                _run(rh, 0, le, o_l)
            _same_outputs(o_l, want_l, 'slot 0')
        rh.pipeline_set_layer(1, None)
        lay['layer'][...] = -7.0
        o_s['image_u8'][...] = 0
        _run(rh, 1, s, o_s)
        while not rh.pipeline_wait(1):
            _run(rh, 1, s, o_s)
        _same_outputs(o_s, want_s, 'slot 1, disarmed')
        assert (lay['layer'] == -7.0).all()
    finally:
        rh.close()


def test_device_pointer_route(cat):
    """rr_render_frames_device reads slot 0's armed table as DEVICE pointers: the bits of the host route."""
    c = cat['seams_low']
    rh = tcc._ctx(c)
    try:
        want = rh.render_frames([c.frame()], want_composite=False, want_layer=True)[0]

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        bg, env, om, dr = dev(c.bg), dev(c.env), dev(c.scene.omega), dev(c.drops.view(np.uint8).reshape(-1))
        rgb = torch.zeros((c.H, c.W, 3), dtype=torch.uint8, device=DEV)
        mask = torch.zeros((c.H, c.W), dtype=torch.float64, device=DEV)
        st = torch.zeros((len(c.drops),), dtype=torch.int32, device=DEV)
        lay = torch.full((2, c.H, c.W, 4), -7.0, dtype=torch.float32, device=DEV)
        sh = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
        fin, fout = (hb.rr_frame_in * 1)(), (hb.rr_frame_out * 1)()
        fin[0].H, fin[0].W, fin[0].He, fin[0].We = c.H, c.W, c.env.shape[0], c.env.shape[1]
        fin[0].bg = fin[0].rainy_bg = bg.data_ptr()
        fin[0].env_xyY, fin[0].omega, fin[0].drops, fin[0].n_drops = env.data_ptr(), om.data_ptr(), dr.data_ptr(), len(c.drops)
        fin[0].opacity_attenuation = 1.0
        fout[0].rainy_rgb, fout[0].mask_f64, fout[0].drop_status = rgb.data_ptr(), mask.data_ptr(), st.data_ptr()
        tab = (hb.rr_layer_out * 2)()
        for k in range(2):
            tab[k].layer, tab[k].shift = lay[k].data_ptr(), sh[k:k + 1].data_ptr()
        arm = hb.rr_pipeline_layer()
        arm.n, arm.frames = 2, ctypes.cast(tab, ctypes.c_void_p)
        torch.cuda.synchronize()
        assert rh.lib.rr_pipeline_set_layer(rh.h, 0, ctypes.byref(arm)) == 0
        with pytest.raises(RuntimeError, match=r'\(-1\).*n = 1.*n = 2'):
            rh.render_frames_device(fin, fout, 1)
        arm.n = 1
        assert rh.lib.rr_pipeline_set_layer(rh.h, 0, ctypes.byref(arm)) == 0
        rh.render_frames_device(fin, fout, 1)
        while not rh.synchronize():
            rh.render_frames_device(fin, fout, 1)
        assert np.array_equal(lay[0].cpu().numpy().view(np.uint32), want['layer'].view(np.uint32)) and float(sh[0]) == want['shift']
        assert bool((lay[1] == -7.0).all()) and float(sh[1]) == -7.0
        assert np.array_equal(rgb.cpu().numpy(), want['image_u8']) and np.array_equal(mask.cpu().numpy(), want['mask'])
        assert np.array_equal(st.cpu().numpy(), want['status'])
    finally:
        rh.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(cat):
    c = cat['seams_low']
    rh = tcc._ctx(c)
    try:
        want = rh.render_frames([c.frame()], want_composite=False, want_layer=True)[0]
        bufs = [dict(layer=np.full((c.H, c.W, 4), -7.0, np.float32), shift=np.full(1, -7.0)) for _ in range(2)]
        tab = (hb.rr_layer_out * 2)()
        for k, b in enumerate(bufs):
            tab[k].layer, tab[k].shift = b['layer'].ctypes.data, b['shift'].ctypes.data
        arm = hb.rr_pipeline_layer()
        arm.n, arm.frames = 2, ctypes.cast(tab, ctypes.c_void_p)

        def err():
            return rh.lib.rr_last_error(rh.h).decode()

        assert rh.lib.rr_pipeline_set_layer(rh.h, 3, ctypes.byref(arm)) == RR_E_ARG and 'slot' in err()          # RR_PIPE_SLOTS == 3
        assert rh.lib.rr_pipeline_set_layer(rh.h, -1, ctypes.byref(arm)) == RR_E_ARG and 'slot' in err()
        bad = hb.rr_pipeline_layer()
        bad.n, bad.frames = 0, ctypes.cast(tab, ctypes.c_void_p)
        assert rh.lib.rr_pipeline_set_layer(rh.h, 0, ctypes.byref(bad)) == RR_E_ARG and 'n must' in err()
        bad.n, bad.frames = 2, None
        assert rh.lib.rr_pipeline_set_layer(rh.h, 0, ctypes.byref(bad)) == RR_E_ARG and 'frames' in err()
        # nothing changed: the slot is still unarmed
        plain = rh.render_frames([c.frame()], want_composite=False)[0]
        _same_outputs(plain, want, 'after the refused arming calls')
        # armed for two frames, a batch of one: refused at submit, nothing enqueued
        assert rh.lib.rr_pipeline_set_layer(rh.h, 0, ctypes.byref(arm)) == 0
        with pytest.raises(RuntimeError, match=r'\(-1\).*n = 2.*n = 1'):
            rh.render_frames([c.frame()], want_composite=False)
        assert all((b['layer'] == -7.0).all() and b['shift'][0] == -7.0 for b in bufs)
        two = rh.render_frames([c.frame(), c.frame()], want_composite=False)
        for b, o in zip(bufs, two):
            assert np.array_equal(b['layer'].view(np.uint32), want['layer'].view(np.uint32)) and b['shift'][0] == want['shift']
            _same_outputs(o, want, 'the valid call behind the refused one')
        rh.pipeline_set_layer(0, None)
        # arming a slot in flight
        o = _outs(rh, c)
        _run(rh, 2, c, o)
        assert rh.lib.rr_pipeline_set_layer(rh.h, 2, ctypes.byref(arm)) == RR_E_STATE and 'in flight' in err()
        while not rh.pipeline_wait(2):
            _run(rh, 2, c, o)
        _same_outputs(o, want, 'slot 2 (never armed)')
        again = rh.render_frames([c.frame()], want_composite=False, want_layer=True)[0]
        assert np.array_equal(again['layer'].view(np.uint32), want['layer'].view(np.uint32)) and again['shift'] == want['shift']
        with pytest.raises(ValueError):
            rh.render_frames([c.frame()], want_layer=1)
    finally:
        rh.close()


# ---- 9. RainAugment(return_layer=True) -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def streaks_db(tmp_path_factory):
    import os
    root = os.path.join(str(tmp_path_factory.mktemp('layerdb')), 'rainstreakdb')
    h.synthetic.write_streak_db(root)
    return root


ODD = types.SimpleNamespace(settings=lambda: {
    "cam_CCD_WH": [641, 359], "cam_WH": [641, 359], "cam_focal": 6, "cam_gain": 20, "cam_f_number": 6.0,
    "cam_focus_plane": 6.0, "cam_exposure": 2, "cam_pos": [1.5, 1.5, 0.3], "cam_lookat": [1.5, 1.5, -1.],
    "cam_up": [0., 1., 0.], "sequences": {}})


@pytest.fixture
def oddcam(monkeypatch):
    monkeypatch.setitem(tga.dbmod.dbs, 'oddcam', ODD)


def _dim_scene(n, H, W, seed):
    """Bytes in 0 .. 63: images scaled to [0, 0.25], so that no blend saturates."""
    bgr, depth = tga._scene(n, H, W, seed=seed)
    return bgr // 4, depth


def _fog_layer(aug, bgr8, depth, rate):
    """rr_prepass_frames_device on the augmenter's own context: the float64 fog layer of the same bytes, [n, H, W, 3] B G R."""
    rh, (n, H, W) = aug._hip, bgr8.shape[:3]
    We = rh._check(rh.lib.rr_envmap_width(rh.h), 'rr_envmap_width')
    img, dep = torch.from_numpy(np.ascontiguousarray(bgr8)).to(DEV), torch.from_numpy(depth).to(DEV)
    out = torch.empty((n, H, W, 3), dtype=torch.float64, device=DEV)
    env = torch.empty((n, H, We, 3), dtype=torch.float64, device=DEV)
    pin, pout = (hb.rr_prepass_in * n)(), (hb.rr_prepass_out * n)()
    fog = aug.plan(rate, [0] * n)['fog']
    for i in range(n):
        pin[i].H, pin[i].W, pin[i].bg, pin[i].depth, pin[i].depth_f64 = H, W, img[i].data_ptr(), dep[i].data_ptr(), 0
        pin[i].in_types = hb.RR_IN_BG_U8
        pin[i].beta_ext, pin[i].beta_hg, pin[i].irr_num, pin[i].irr_den = [float(v) for v in fog[i]]
        pout[i].rainy_bg, pout[i].env_xyY, pout[i].out_types = out[i].data_ptr(), env[i].data_ptr(), 0
    torch.cuda.synchronize()
    rh._check(rh.lib.rr_prepass_frames_device(rh.h, n, pin, pout, None), 'rr_prepass_frames_device')
    rh.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('dataset, seq', [('kitti', 'data_object/training'), ('nuscenes', None), ('oddcam', None)])
def test_augment_returns_the_layer(built, streaks_db, oddcam, dataset, seq):
    aug = augment.RainAugment(dataset, streaks_db=streaks_db, sequence=seq, return_layer=True)
    plain = augment.RainAugment(dataset, streaks_db=streaks_db, sequence=seq)
    try:
        H, W = aug.frame_size()
        bgr, depth = _dim_scene(2, H, W, seed=40)
        img, dep, idx = tga._planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV), [4, 11]
        rainy, mask, layer = aug(img, dep, 25, idx)
        r0, m0 = plain(img, dep, 25, idx)
        assert torch.equal(rainy, r0) and torch.equal(mask, m0) and float(mask.max()) > 0
        assert layer.colour.shape == (2, 3, H, W) and layer.transmittance.shape == (2, 1, H, W) and layer.background.shape == (2, 3, H, W)
        assert layer.shift.shape == (2,) and layer.shift.dtype == torch.float64 and layer.shift.device == img.device
        assert layer.colour.dtype == layer.transmittance.dtype == layer.background.dtype == torch.float32
        assert layer.colour.data_ptr() == layer.planes.data_ptr() and layer.transmittance.data_ptr() == layer.planes.data_ptr() + 3 * H * W * 4
        # the layer over the rain-free target is the rainy image
        v = layer.over(layer.background)
        d = ((v.double() * 255.0).to(torch.uint8).int() - rainy.int()).abs()
        print('%s: max |d| %d LSB, shift %s' % (dataset, int(d.max()), layer.shift.cpu().numpy()))
        assert int(d.max()) <= 1
        dry = mask == 0
        assert bool((layer.transmittance[dry] == 1).all()) and bool((layer.colour[dry.expand(-1, 3, -1, -1)] == 0).all())
        assert float(layer.transmittance.min()) < 1 and float(layer.colour.max()) > 0
        # the transmittance knows nothing of the images
        other, _ = _dim_scene(2, H, W, seed=77)
        _, m2, layer2 = aug(tga._planar(other).to(DEV), dep, 25, idx)
        assert torch.equal(layer2.transmittance, layer.transmittance) and torch.equal(m2, mask)
        assert not torch.equal(layer2.background, layer.background)
        # the background is the pre-pass' fog layer: float32 values in [0, 1], each the float64 one rounded once (<= 2^-25)
        fog = _fog_layer(aug, bgr, depth, 25)[..., ::-1].transpose(0, 3, 1, 2)
        e = np.abs(layer.background.cpu().numpy().astype(np.float64) - fog).max()
        print('%s: background vs the float64 fog layer: %.3g' % (dataset, e))
        assert e <= 2.0 ** -25
    finally:
        aug.close()
        plain.close()


def test_augment_layer_does_not_depend_on_dtype_or_layout(built, streaks_db, oddcam):
    """Bytes 0 and 255 are 0.0 and 1.0 in every dtype: all batches hold the same numbers."""
    aug = augment.RainAugment('oddcam', streaks_db=streaks_db, return_layer=True)
    try:
        H, W = aug.frame_size()
        bgr, depth = tga._scene(2, H, W, seed=5)
        x8 = tga._planar(((bgr > 127) * 255).astype(np.uint8)).to(DEV)
        dep, idx = torch.from_numpy(depth).to(DEV), [3, 8]
        xf = x8.float() / 255.0
        _, mask, want = aug(xf, dep, 50, idx)
        assert want.planes.is_contiguous() and float(mask.max()) > 0
        CL = torch.channels_last
        for x in (x8, x8.contiguous(memory_format=CL), xf.contiguous(memory_format=CL), xf.half(), xf.half().contiguous(memory_format=CL),
                  xf.bfloat16()):
            rainy, m, got = aug(x, dep, 50, idx)
            assert rainy.dtype == x.dtype and rainy.stride() == x.stride() and torch.equal(m, mask)
            assert got.planes.dtype == torch.float32 and got.planes.is_contiguous() and got.background.is_contiguous()
            assert torch.equal(got.planes, want.planes) and torch.equal(got.background, want.background), (x.dtype, x.stride())
            assert torch.equal(got.shift, want.shift) or x.dtype != torch.float32
    finally:
        aug.close()


def test_augment_layer_with_a_lens_is_the_streaks_alone(built, streaks_db, oddcam):
    lens = importlib.import_module('rain-rendering_amd.tools.lens')
    L = lens.LensDrops(359, 641, count=12, seed=3)
    a = augment.RainAugment('oddcam', streaks_db=streaks_db, return_layer=True)
    b = augment.RainAugment('oddcam', streaks_db=streaks_db, return_layer=True, lens=L, return_lens_alpha=True)
    try:
        bgr, depth = _dim_scene(2, 359, 641, seed=9)
        img, dep = tga._planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV)
        rainy, mask, want = a(img, dep, 25, [4, 31])
        out = b(img, dep, 25, [4, 31])
        assert len(out) == 4 and float(out[2].max()) > 0 and not torch.equal(out[0], rainy) and torch.equal(out[1], mask)
        for k in ('planes', 'background', 'shift'):
            assert torch.equal(getattr(out[3], k), getattr(want, k)), k
    finally:
        a.close()
        b.close()


def test_augment_layer_at_the_render_size(built, streaks_db, monkeypatch):
    tgr = importlib.import_module('test_gpu_input_resize')
    tgr._small_camera(monkeypatch, 2)                                    # a 160 x 96 sensor rendered at scale 2: 48 x 80 frames
    SH, SW = tgr.SH, tgr.SW
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', source_size=(SH, SW), return_layer=True)
    try:
        H, W = aug.frame_size()
        assert (H, W) == (SH // 2, SW // 2)
        bgr, _ = _dim_scene(2, SH, SW, seed=5)
        _, depth = tga._scene(2, H, W, seed=5)
        rainy, mask, layer = aug(tga._planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV), 25, [0, 1])
        assert rainy.shape == (2, 3, H, W) and layer.planes.shape == (2, 4, H, W) and layer.background.shape == (2, 3, H, W)
        d = ((layer.over(layer.background).double() * 255.0).to(torch.uint8).int() - rainy.int()).abs()
        assert int(d.max()) <= 1 and float(mask.max()) > 0 and float(layer.transmittance.min()) < 1
    finally:
        aug.close()


def test_augment_layer_of_a_rig(built, streaks_db, oddcam):
    rigmod = importlib.import_module('rain-rendering_amd.rig')
    kw = dict(streaks_db=streaks_db, particle_model='rig', rig=rigmod.Rig.stereo(0.54), return_layer=True)
    both, right = augment.RainAugment('oddcam', **kw), augment.RainAugment('oddcam', views=[1], **kw)
    try:
        bgr, depth = _dim_scene(4, 359, 641, seed=13)
        img = tga._planar(bgr).reshape(2, 2, 3, 359, 641).to(DEV)
        dep = torch.from_numpy(depth).reshape(2, 2, 359, 641).to(DEV)
        rainy, mask, layer = both(img, dep, 25, [2, 6])
        assert layer.colour.shape == (2, 2, 3, 359, 641) and layer.transmittance.shape == (2, 2, 1, 359, 641)
        assert layer.background.shape == (2, 2, 3, 359, 641) and layer.shift.shape == (2, 2)
        r1, m1, one = right(img[:, 1:2], dep[:, 1:2], 25, [2, 6])
        assert torch.equal(r1, rainy[:, 1:2]) and torch.equal(m1, mask[:, 1:2]) and float(m1.max()) > 0
        assert torch.equal(one.planes, layer.planes[:, 1:2]) and torch.equal(one.background, layer.background[:, 1:2])
        assert torch.equal(one.shift, layer.shift[:, 1:2])
        d = ((layer.over(layer.background).double() * 255.0).to(torch.uint8).int() - rainy.int()).abs()
        assert int(d.max()) <= 1
    finally:
        both.close()
        right.close()
