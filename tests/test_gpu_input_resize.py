"""GPU tier of the render-scale resize of the inputs (rr_set_input_resize): the kernels k_resize_in / k_resize_depth
against numpy (common/imgops.py resize_linear) for every case and kind of tests/resize_cases.py, then the armed entry points
against the unarmed ones fed the host-resized arrays, the driver's --device_resize against the default route, and
RainAugment(source_size=) against the driver's files.  Everything bit for bit: the resize is + - * / floor in IEEE float64 without
contraction, float32 depth one rounding of it, and behind the stage the call is the float64-image route it always was."""
import importlib
import os

import numpy as np
import pytest
import torch                                    # (before the library is loaded: torch brings its own HIP runtime)

import helpers as h
import pngrows_cases as pr
import resize_cases as rc
import test_gpu_prepass as tp

pytestmark = pytest.mark.gpu

imgops = rc.imgops
H, W = 48, 80                                   # the render size of the pipeline tests: case (b) image, case (e) depth
KEYS = ('image_u8', 'mask', 'mask_i32', 'status')


@pytest.fixture(scope="module")
def ctx(built):
    rh = h.hb.RainHip(0)
    yield rh
    rh.close()


def _where(a, b):
    return np.argwhere(a != b)[:4].tolist()


@pytest.mark.parametrize("kind", rc.IMAGE_KINDS)
@pytest.mark.parametrize("case", sorted(rc.IMAGE_CASES))
def test_image_kernel_equals_numpy(ctx, case, kind):
    (dh, dw), (sh, sw) = rc.IMAGE_CASES[case]
    arr, planar, _ = rc.image_input(case, kind)
    ctx.set_input_resize(sh, sw, sh, sw)
    ctx.profile(True)
    ctx.profile_reset()
    got, none = ctx.resize_inputs(dh, dw, images=arr, planar=planar)
    launches = ctx.profile_read().get('k_resize_in', (0, 0.0))[0]
    ctx.profile(False)
    ctx.set_input_resize()
    want = rc.image_want(case, kind)
    assert none is None and launches == 1 and got.shape == want.shape and got.dtype == np.float64
    for f in range(rc.N):
        assert np.array_equal(got[f], want[f]), (case, kind, f, _where(got[f], want[f]))


@pytest.mark.parametrize("kind", rc.DEPTH_KINDS)
@pytest.mark.parametrize("case", sorted(rc.DEPTH_CASES))
def test_depth_kernel_equals_numpy(ctx, case, kind):
    (dh, dw), (sh, sw) = rc.DEPTH_CASES[case]
    arr = rc.depth_input(case, kind)
    ctx.set_input_resize(sh, sw, sh, sw)
    ctx.profile(True)
    ctx.profile_reset()
    none, got = ctx.resize_inputs(dh, dw, depth=arr)
    launches = ctx.profile_read().get('k_resize_depth', (0, 0.0))[0]
    ctx.profile(False)
    ctx.set_input_resize()
    want = rc.depth_want(case, kind)
    assert none is None and launches == 1 and got.shape == want.shape and got.dtype == np.float32
    for f in range(rc.N):
        assert np.array_equal(got[f], want[f]), (case, kind, f, _where(got[f], want[f]))


def test_both_sides_in_one_call_and_the_setter_checks(ctx):
    """Image and depth of different source sizes in one call; sizes the setter refuses; the stage unarmed."""
    (dh, dw), (sh, sw) = rc.IMAGE_CASES['b']
    _, (eh, ew) = rc.DEPTH_CASES['e']
    ctx.set_input_resize(sh, sw, eh, ew)
    bg, dep = ctx.resize_inputs(dh, dw, images=rc.image_input('b', 'bgr_u8')[0], depth=rc.depth_input('e', 'u16'))
    assert np.array_equal(bg, rc.image_want('b', 'bgr_u8')) and np.array_equal(dep, rc.depth_want('e', 'u16'))
    for bad in ((0, sw, eh, ew), (sh, -1, eh, ew), (sh, sw, 16385, ew), (sh, sw, eh, 0)):
        with pytest.raises(RuntimeError, match=r'\(-1\)'):
            ctx.set_input_resize(*bad)
    bg2, _ = ctx.resize_inputs(dh, dw, images=rc.image_input('b', 'bgr_u8')[0])      # a refused call leaves the armed sizes alone
    assert np.array_equal(bg2, bg)
    ctx.set_input_resize(16384, 16384, 1, 1)
    ctx.set_input_resize()
    with pytest.raises(RuntimeError, match='rr_set_input_resize first'):
        ctx.resize_inputs(dh, dw, images=rc.image_input('b', 'bgr_u8')[0])


def _render_context(sc):
    rh = h.hb.RainHip(0)
    rh.set_streak_db(sc.db.streaks_light)
    rh.set_camera(sc.cam)
    rh.set_colormap(imgops.viridis_lut())
    consts, We = tp._setup(rh, H, W, 25)
    return rh, consts


@pytest.fixture(scope="module")
def scene(tmp_path_factory, built):
    """Three frames of ~100 drops at the render size, their source-size inputs (case b image, case e depth) and the host-resized
    arrays the unarmed call takes."""
    sc = h.Scene(tmp_path_factory.mktemp('resize_scene'), H, W, 100, n_frames=rc.N, seed0=77)
    return dict(sc=sc, bgr=rc.image_bytes('b'), d16=rc.scene_depth('e'), drops=[sc.product_drops(i) for i in range(rc.N)],
                bg=[imgops.resize_linear(f / 255.0, W, H) for f in rc.image_bytes('b')],
                depth=[imgops.resize_linear(rc.depth_metres(d), W, H).astype(np.float32) for d in rc.scene_depth('e')])


def _outs(drops, png):
    o = dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W)), mask_i32=np.zeros((H, W), np.int32), status=np.zeros(len(drops), np.int32))
    if png:
        o.update(rainy_png=np.zeros(H * (1 + 4 * W), np.uint8), mask_png=np.zeros(H * (1 + 4 * W), np.uint8))
    return o


def test_armed_pipeline_equals_unarmed_on_host_resized_inputs(scene):
    sc = scene['sc']
    (sh, sw), (eh, ew) = rc.IMAGE_CASES['b'][1], rc.DEPTH_CASES['e'][1]
    rh, consts = _render_context(sc)
    try:
        common = [dict(fog=consts, omega=sc.omega, drops=scene['drops'][i]) for i in range(rc.N)]
        want = rh.pipeline_frames([dict(c, bg=scene['bg'][i], depth=scene['depth'][i]) for i, c in enumerate(common)])
        assert all(len(c['drops']) > 40 for c in common) and all(o['mask'].max() > 0 for o in want)
        rh.set_input_resize(sh, sw, eh, ew)
        rh.profile(True)
        rh.profile_reset()
        got = rh.pipeline_frames([dict(c, bg_u8=scene['bgr'][i], depth=scene['d16'][i], render_shape=(H, W)) for i, c in enumerate(common)])
        prof = rh.profile_read()
        rh.profile(False)
        assert prof.get('k_resize_in', (0,))[0] == 1 and prof.get('k_resize_depth', (0,))[0] == 1, prof
        for i in range(rc.N):
            for k in KEYS:
                assert np.array_equal(got[i][k], want[i][k]), (i, k)
        # float32 metres of the source size instead of the samples: the same map behind the stage
        got = rh.pipeline_frames([dict(c, bg_u8=scene['bgr'][i], depth=rc.depth_metres(scene['d16'][i]), render_shape=(H, W))
                                  for i, c in enumerate(common)])
        for i in range(rc.N):
            for k in KEYS:
                assert np.array_equal(got[i][k], want[i][k]), (i, k)
        # an interleaved float image while armed is refused
        with pytest.raises(RuntimeError, match=r'\(-1\)'):
            rh.pipeline_frames([dict(common[0], bg=scene['bg'][0], depth=scene['d16'][0], render_shape=(H, W), depth_shape=(eh, ew))])
        # the files' filtered scanlines through rr_pipeline_submit: un-filtered at the source size, PNG payloads included
        rh.set_input_resize()
        ref = [_outs(c['drops'], True) for c in common]
        rh.pipeline_submit(0, [dict(c, bg=scene['bg'][i], depth=scene['depth'][i]) for i, c in enumerate(common)], ref)
        assert rh.pipeline_wait(0)
        rh.set_input_resize(sh, sw, eh, ew)
        plans_i, plans_d = pr.plans(sh, 5)[-2:] + pr.plans(sh, 6)[-1:], pr.plans(eh, 7)[-2:] + pr.plans(eh, 8)[-1:]
        rows = [dict(c, bg_png_rows=pr.png_filter(pr.image_samples(scene['bgr'][i]), plans_i[i]).ravel(), shape=(sh, sw),
                     depth_png_rows=pr.png_filter(pr.depth_samples(scene['d16'][i]), plans_d[i]).ravel(), depth_shape=(eh, ew),
                     render_shape=(H, W)) for i, c in enumerate(common)]
        outs = [_outs(c['drops'], True) for c in common]
        rh.profile(True)
        rh.profile_reset()
        rh.pipeline_submit(1, rows, outs)
        assert rh.pipeline_wait(1)
        prof = rh.profile_read()
        rh.profile(False)
        assert prof.get('k_png_unfilter', (0,))[0] == 1 and prof.get('k_resize_in', (0,))[0] == 1, prof
        for i in range(rc.N):
            for k in KEYS + ('rainy_png', 'mask_png'):
                assert np.array_equal(outs[i][k], ref[i][k]), (i, k)
            assert np.array_equal(ref[i]['image_u8'], want[i]['image_u8']) and ref[i]['rainy_png'].any()
    finally:
        rh.close()


def test_disarming_restores_the_context(scene):
    sc = scene['sc']
    (sh, sw), (eh, ew) = rc.IMAGE_CASES['b'][1], rc.DEPTH_CASES['e'][1]
    bg8 = [np.round(b * 255).astype(np.uint8) for b in scene['bg']]
    outs = []
    for armed_before in (True, False):
        rh, consts = _render_context(sc)
        try:
            common = [dict(fog=consts, omega=sc.omega, drops=scene['drops'][i]) for i in range(rc.N)]
            if armed_before:
                rh.set_input_resize(sh, sw, eh, ew)
                rh.pipeline_frames([dict(c, bg_u8=scene['bgr'][i], depth=scene['d16'][i], render_shape=(H, W)) for i, c in enumerate(common)])
                rh.set_input_resize()
            outs.append(rh.pipeline_frames([dict(c, bg_u8=bg8[i], depth=scene['depth'][i]) for i, c in enumerate(common)]))
        finally:
            rh.close()
    for i in range(rc.N):
        for k in KEYS:
            assert np.array_equal(outs[0][i][k], outs[1][i][k]), (i, k)


# ---- the driver: main.py --device_resize writes the files of the default route --------------------------------------------------------
from PIL import Image                                                # noqa: E402

main_mod = importlib.import_module('rain-rendering_amd.main')
augment = importlib.import_module('rain-rendering_amd.augment')
SH, SW, NF = 96, 160, 4                                              # the trees' images; render_scale 2 -> 48 x 80 frames
DEV = torch.device('cuda', 0)


def _small_camera(mp, depth_scale):
    """The KITTI plug-in with a 160 x 96 sensor rendered at half resolution (what config/cityscapes.py does at its own size)."""
    kitti = importlib.import_module('rain-rendering_amd.config.kitti')
    plain = kitti.settings

    def scaled():
        st = dict(plain())
        st.update(render_scale=2, depth_scale=depth_scale, cam_WH=[SW, SH], cam_CCD_WH=[SW, SH])
        return st
    mp.setattr(kitti, 'settings', scaled)


def _tree(tmp, dh, dw):
    """NF frames of 96 x 160 with noise depth maps of dh x dw (2 .. 80 m), a streak database and a particle file."""
    src = os.path.join(tmp, 'source')
    img_dir, dep_dir = h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), NF, SH, SW)
    for i in range(NF):
        d = np.random.RandomState(900 + i).randint(512, 20480, (dh, dw)).astype(np.uint16)
        Image.fromarray(d).save(os.path.join(dep_dir, '%06d.png' % i))
    h.synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
    xml = os.path.join(tmp, 'particles', 'kitti', 'data_object', 'rain', '25mm', 'sim_camera0.xml')
    h.synthetic.write_particles_xml(xml, h.synthetic.simulate_particles(2, 150, SW, SH))
    return src, img_dir, dep_dir


def _main(tmp, src, out, flags):
    gen = main_mod.main(['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', os.path.join(tmp, 'rainstreakdb'),
                         '-i', '25', '--output', os.path.join(tmp, out), '--noverbose'] + flags)
    assert len(gen.stats) == NF and gen.timing[0].get('route') == 'native'
    return os.path.join(tmp, out, 'kitti', 'data_object', 'training', 'rain', '25mm')


@pytest.mark.parametrize("device_particles", [False, True])
@pytest.mark.parametrize("dh,dw,depth_scale", [(48, 80, 2), (96, 160, 1)])
def test_driver_flag_writes_byte_identical_files(tmp_path, built, monkeypatch, dh, dw, depth_scale, device_particles):
    tmp = str(tmp_path)
    src, _, _ = _tree(tmp, dh, dw)
    _small_camera(monkeypatch, depth_scale)
    monkeypatch.setenv('RAIN_BATCH', '3')                              # two batches, a ragged last one
    flags = ['--device_particles'] if device_particles else []
    want = _main(tmp, src, 'out_default', flags)
    got = _main(tmp, src, 'out_resize', flags + ['--device_resize'])
    rained = 0
    for kind in ('rainy_image', 'rain_mask'):
        for i in range(NF):
            a = open(os.path.join(want, kind, '%06d.png' % i), 'rb').read()
            b = open(os.path.join(got, kind, '%06d.png' % i), 'rb').read()
            assert a == b, (kind, i)
        img = np.array(Image.open(os.path.join(got, kind, '%06d.png' % 0)))
        assert img.shape == (SH // 2, SW // 2, 4)
        rained += int(img[..., :3].std() > 0)
    assert rained == 2


# ---- RainAugment(source_size=): full-size tensors in, the driver's files out -----------------------------------------------------------
def test_augment_source_size_equals_the_driver_files(tmp_path, built, monkeypatch):
    import test_gpu_augment as tga
    tmp = str(tmp_path)
    src, img_dir, dep_dir = _tree(tmp, 48, 80)
    _small_camera(monkeypatch, 2)
    out = _main(tmp, src, 'out', ['--device_particles', '--device_resize'])
    rgb = np.stack([np.array(Image.open(os.path.join(img_dir, '%06d.png' % i)).convert('RGB')) for i in range(NF)])
    depth = np.stack([np.array(Image.open(os.path.join(dep_dir, '%06d.png' % i))).astype(np.float32) / np.float32(256.) for i in range(NF)])
    idx = list(range(NF))
    aug = augment.RainAugment('kitti', streaks_db=os.path.join(tmp, 'rainstreakdb'), sequence='data_object/training', source_size=(SH, SW))
    try:
        assert aug.frame_size() == (SH // 2, SW // 2) and aug.depth_size == (SH // 2, SW // 2)
        planar = torch.from_numpy(rgb.transpose(0, 3, 1, 2).copy()).to(DEV)
        rainy8, mask8 = aug(planar, torch.from_numpy(depth).to(DEV), 25, idx)
        assert rainy8.shape == (NF, 3, SH // 2, SW // 2) and rainy8.dtype == torch.uint8 and mask8.shape == (NF, 1, SH // 2, SW // 2)
        rainy8, mask8 = rainy8.cpu().numpy(), mask8.cpu().numpy()
        for i in range(NF):                                           # the RGB of the PNG the run wrote
            got = np.array(Image.open(os.path.join(out, 'rainy_image', '%06d.png' % i)))[..., :3]
            assert np.array_equal(rainy8[i].transpose(1, 2, 0), got), i
        # ... and image and mask of rr_pipeline_submit on the same records, fed the host-resized float64 image
        p = aug.plan(25, idx)
        bgr = rgb[..., ::-1]
        ref = tga._pipeline(aug, p, np.stack([imgops.resize_linear(f / 255.0, SW // 2, SH // 2) for f in bgr]), depth)
        for i, (img_u8, m64) in enumerate(ref):
            assert np.array_equal(rainy8[i].transpose(1, 2, 0), img_u8) and np.array_equal(mask8[i, 0], m64.astype(np.float32)), i
            assert m64.max() > 0, i
        # float32 tensors are widened, not re-quantised: the same mask, the image of the pipeline fed the widened floats resized
        f32 = np.random.RandomState(5).uniform(0, 1, bgr.shape).astype(np.float32)
        rainyf, maskf = aug(tga._planar(f32).to(DEV), torch.from_numpy(depth).to(DEV)[:, None], 25, idx)
        assert rainyf.dtype == torch.float32
        rainyf, maskf = rainyf.cpu().numpy(), maskf.cpu().numpy()
        ref = tga._pipeline(aug, p, np.stack([imgops.resize_linear(f.astype(np.float64), SW // 2, SH // 2) for f in f32]), depth)
        for i, (img_u8, m64) in enumerate(ref):
            assert np.array_equal(rainyf[i].transpose(1, 2, 0), img_u8.astype(np.float32) / np.float32(255.0)), i
            assert np.array_equal(maskf[i, 0], mask8[i, 0]) and np.array_equal(maskf[i, 0], m64.astype(np.float32)), i
    finally:
        aug.close()
    # depth maps of their own size: depth_size
    aug = augment.RainAugment('kitti', streaks_db=os.path.join(tmp, 'rainstreakdb'), sequence='data_object/training', source_size=(SH, SW),
                              depth_size=(24, 40))
    try:
        small = np.ascontiguousarray(depth[:2, ::2, ::2])
        rainy, mask = aug(planar[:2], torch.from_numpy(small).to(DEV), 25, idx[:2])
        up = np.stack([imgops.resize_linear(d, SW // 2, SH // 2).astype(np.float32) for d in small])
        ref = tga._pipeline(aug, aug.plan(25, idx[:2]), np.stack([imgops.resize_linear(f / 255.0, SW // 2, SH // 2) for f in bgr[:2]]), up)
        for i, (img_u8, m64) in enumerate(ref):
            assert np.array_equal(rainy[i].cpu().numpy().transpose(1, 2, 0), img_u8) and np.array_equal(mask[i, 0].cpu().numpy(), m64.astype(np.float32)), i
    finally:
        aug.close()
