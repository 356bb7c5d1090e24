"""GPU tier of the input-resize catalogue (tests/resize_catalogue.py): k_resize_in<KIND> / k_resize_depth<KIND> through
rr_resize_inputs_device for every case and every kind the stage has -- segments behind the first, the staged / direct choice at its
limit, buffers that start off a 16-byte boundary, the three store shapes -- against common/imgops.py resize_linear on the float64
values of the input, as bit patterns; guard elements around the outputs and the input buffer checked afterwards.  Then the callers
that compute lo, hi and strides of their own at a two-segment render width: the armed pipeline entry points against the unarmed ones
on host-resized inputs, and RainAugment(source_size=) for the half types in both layouts.  Nothing here has a tolerance."""
import importlib

import numpy as np
import pytest
import torch                                    # (before the library is loaded: torch brings its own HIP runtime)

import helpers as h
import pngrows_cases as pr
import resize_catalogue as cat
import test_gpu_prepass as tp

pytestmark = pytest.mark.gpu

imgops = cat.imgops
GUARD = 4                                       # elements before frame 0 and behind the last frame: 32 / 16 bytes, the outputs stay 16-byte aligned
KEYS = ('image_u8', 'mask', 'mask_i32', 'status')


@pytest.fixture(scope="module")
def ctx(built):
    rh = h.hb.RainHip(0)
    yield rh
    rh.close()


def _run(ctx, name, **sides):
    """One profiled call of the stage alone; (bg, depth, info, launches per scope)."""
    ctx.profile(True)
    ctx.profile_reset()
    try:
        bg, dep, info = ctx.resize_inputs(guard=GUARD, **sides)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    return bg, dep, info, {k: prof.get(k, (0, 0.0))[0] for k in ('k_resize_in', 'k_resize_depth')}


@pytest.mark.parametrize("name", list(cat.CASES))
def test_kernel_equals_numpy_bit_for_bit(ctx, name):
    c = cat.CASES[name]
    k = cat.KINDS[c.kind]
    arr, _ = cat.case_input(name)
    want = cat.case_want(name)
    ctx.set_input_resize(c.sH, c.sW, c.sH, c.sW)
    try:
        if k.image:
            got, none, info, launches = _run(ctx, name, H=c.H, W=c.W, images=arr, kind=k.code, in_offset=c.offset)
            side, guard = 'images_buffer', 'bg_guard'
            assert launches == {'k_resize_in': 1, 'k_resize_depth': 0}
        else:
            none, got, info, launches = _run(ctx, name, H=c.H, W=c.W, depth=arr, in_offset=c.offset)
            side, guard = 'depth_buffer', 'depth_guard'
            assert launches == {'k_resize_in': 0, 'k_resize_depth': 1}
    finally:
        ctx.set_input_resize()
    assert none is None and got.shape == want.shape and got.dtype == want.dtype
    for f in range(cat.N):
        assert not cat.mismatches(got[f], want[f]), (name, f, cat.mismatches(got[f], want[f]))
    front, back = info[guard]
    assert front.size == back.size == GUARD * got.dtype.itemsize and (front == 0xA5).all() and (back == 0xA5).all(), name
    before, after = info[side]
    assert before.size == arr.nbytes + 48 and np.array_equal(before, after), name
    assert np.array_equal(before[16 + c.offset:16 + c.offset + arr.nbytes], arr.view(np.uint8).reshape(-1))


def test_both_sides_in_one_call_at_two_segments(ctx):
    """An interleaved float16 image and a uint16 depth map in one call, three segments each behind the stage."""
    ci, cd = cat.CASES['seg1025-rgb_f16'], cat.CASES['seg1025-u16']
    assert (ci.H, ci.W) == (cd.H, cd.W) and len(cat.predict(ci.kind, ci.H, ci.W, ci.sH, ci.sW).segments) == 3
    ctx.set_input_resize(ci.sH, ci.sW, cd.sH, cd.sW)
    try:
        bg, dep, info, launches = _run(ctx, 'both', H=ci.H, W=ci.W, images=cat.case_input(ci.name)[0], kind=cat.KINDS[ci.kind].code,
                                       depth=cat.case_input(cd.name)[0])
    finally:
        ctx.set_input_resize()
    assert launches == {'k_resize_in': 1, 'k_resize_depth': 1}
    assert not cat.mismatches(bg, cat.case_want(ci.name)) and not cat.mismatches(dep, cat.case_want(cd.name))
    for g in info['bg_guard'] + info['depth_guard']:
        assert g.size and (g == 0xA5).all()


def test_the_new_kinds_check_their_arguments(ctx):
    """A pointer off its element size and a kind outside the enum are RR_E_ARG with nothing run; a valid call works afterwards."""
    c = cat.CASES['seg513-rgb_f16']
    arr = cat.case_input(c.name)[0]
    ctx.set_input_resize(c.sH, c.sW, c.sH, c.sW)
    try:
        for kind, off in ((h.hb.RR_RESIZE_RGB_F16, 1), (h.hb.RR_RESIZE_RGB_BF16_PLANAR, 3), (h.hb.RR_RESIZE_RGB_F32, 2), (9, 0), (-1, 0)):
            with pytest.raises(RuntimeError, match=r'\(-1\)'):
                ctx.resize_inputs(c.H, c.W, images=arr, kind=kind, in_offset=off)
        got = ctx.resize_inputs(c.H, c.W, images=arr, kind=h.hb.RR_RESIZE_RGB_F16, in_offset=2)[0]      # aligned to the element: taken
        assert not cat.mismatches(got, cat.case_want(c.name))
    finally:
        ctx.set_input_resize()


# ---- the pipeline at a two-segment render width: its own lo, hi and strides -----------------------------------------------------------
H, W = 24, 520                                  # render size; 48 x 1040 bytes and a 12 x 260 uint16 depth map in
SH, SW, DH, DW = 48, 1040, 12, 260


@pytest.fixture(scope="module")
def scene(tmp_path_factory, built):
    sc = h.Scene(tmp_path_factory.mktemp('resize_wide_scene'), H, W, 100, n_frames=cat.N, seed0=78)
    rng = np.random.RandomState(780)
    bgr = rng.randint(0, 256, (cat.N, SH, SW, 3)).astype(np.uint8)
    bgr[:, 0, 0], bgr[:, -1, -1] = 0, 255
    d16 = rng.randint(512, 65536, (cat.N, DH, DW)).astype(np.uint16)      # nothing nearer than 2 m: the fog layer divides by the depth
    d16[:, -1, -1] = 65535
    metres = d16.astype(np.float32) / np.float32(256.0)
    return dict(sc=sc, bgr=bgr, d16=d16, drops=[sc.product_drops(i) for i in range(cat.N)],
                bg=[imgops.resize_linear(f / 255.0, W, H) for f in bgr],
                depth=[imgops.resize_linear(m, W, H).astype(np.float32) for m in metres])


def _outs(drops):
    return dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W)), mask_i32=np.zeros((H, W), np.int32), status=np.zeros(len(drops), np.int32),
                rainy_png=np.zeros(H * (1 + 4 * W), np.uint8), mask_png=np.zeros(H * (1 + 4 * W), np.uint8))


def test_armed_pipeline_at_two_segments_equals_unarmed_on_host_resized_inputs(scene):
    sc = scene['sc']
    assert len(cat.predict('bgr_u8', H, W, SH, SW).segments) == 2 and len(cat.predict('u16', H, W, DH, DW).segments) == 2
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        rh.set_colormap(imgops.viridis_lut())
        consts, We = tp._setup(rh, H, W, 25)
        common = [dict(fog=consts, omega=sc.omega, drops=scene['drops'][i]) for i in range(cat.N)]
        want = rh.pipeline_frames([dict(c, bg=scene['bg'][i], depth=scene['depth'][i]) for i, c in enumerate(common)])
        assert all(len(c['drops']) > 40 for c in common) and all(o['mask'].max() > 0 for o in want)
        rh.set_input_resize(SH, SW, DH, DW)
        rh.profile(True)
        rh.profile_reset()
        got = rh.pipeline_frames([dict(c, bg_u8=scene['bgr'][i], depth=scene['d16'][i], render_shape=(H, W)) for i, c in enumerate(common)])
        prof = rh.profile_read()
        rh.profile(False)
        assert prof.get('k_resize_in', (0,))[0] == 1 and prof.get('k_resize_depth', (0,))[0] == 1, prof
        for i in range(cat.N):
            for k in KEYS:
                assert np.array_equal(got[i][k], want[i][k]), (i, k)
        # the files' filtered scanlines through rr_pipeline_submit: un-filtered at the source size, PNG payloads included
        rh.set_input_resize()
        ref = [_outs(c['drops']) for c in common]
        rh.pipeline_submit(0, [dict(c, bg=scene['bg'][i], depth=scene['depth'][i]) for i, c in enumerate(common)], ref)
        assert rh.pipeline_wait(0)
        rh.set_input_resize(SH, SW, DH, DW)
        plans_i, plans_d = pr.plans(SH, 5)[-2:] + pr.plans(SH, 6)[-1:], pr.plans(DH, 7)[-2:] + pr.plans(DH, 8)[-1:]
        rows = [dict(c, bg_png_rows=pr.png_filter(pr.image_samples(scene['bgr'][i]), plans_i[i]).ravel(), shape=(SH, SW),
                     depth_png_rows=pr.png_filter(pr.depth_samples(scene['d16'][i]), plans_d[i]).ravel(), depth_shape=(DH, DW),
                     render_shape=(H, W)) for i, c in enumerate(common)]
        outs = [_outs(c['drops']) for c in common]
        rh.profile(True)
        rh.profile_reset()
        rh.pipeline_submit(1, rows, outs)
        assert rh.pipeline_wait(1)
        prof = rh.profile_read()
        rh.profile(False)
        assert prof.get('k_png_unfilter', (0,))[0] == 1 and prof.get('k_resize_in', (0,))[0] == 1 and prof.get('k_resize_depth', (0,))[0] == 1, prof
        for i in range(cat.N):
            for k in KEYS + ('rainy_png', 'mask_png'):
                assert np.array_equal(outs[i][k], ref[i][k]), (i, k)
            assert np.array_equal(ref[i]['image_u8'], want[i]['image_u8']) and ref[i]['rainy_png'].any()
    finally:
        rh.close()


# ---- RainAugment(source_size=): the half types, planar and channels-last, at a source two segments wide -----------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_augment_half_types_through_a_two_segment_resize(built, tmp_path, monkeypatch, dtype):
    tgf = importlib.import_module('test_gpu_tensor_formats')
    augment = tgf.augment
    kitti = importlib.import_module('rain-rendering_amd.config.kitti')
    plain = kitti.settings

    def scaled():                                                        # a 1040 x 48 sensor rendered at scale 2: 24 x 520 frames
        st = dict(plain())
        st.update(render_scale=2, depth_scale=2, cam_WH=[SW, SH], cam_CCD_WH=[SW, SH])
        return st
    monkeypatch.setattr(kitti, 'settings', scaled)
    db = str(tmp_path / 'rainstreakdb')
    h.synthetic.write_streak_db(db)
    aug = augment.RainAugment('kitti', streaks_db=db, sequence='data_object/training', source_size=(SH, SW))
    try:
        assert aug.frame_size() == (H, W)
        idx = [0, 1, 2]
        dep = tgf._depth(3, H, W, seed=6).to(tgf.DEV)
        xh = tgf._images(dtype, 3, SH, SW, seed=6).to(tgf.DEV)
        want, mask = aug(xh.float(), dep, 25, idx)                       # planar float32 on the widened values, narrowed
        assert want.shape == (3, 3, H, W) and all(float(mask[i].max()) > 0 for i in range(3))
        for x in (xh, xh.contiguous(memory_format=tgf.CL)):
            r, m = aug(x, dep, 25, idx)
            assert r.dtype == dtype and torch.equal(r, want.to(dtype)) and torch.equal(m, mask), (dtype, x.stride())
        assert r.is_contiguous(memory_format=tgf.CL) and not r.is_contiguous()
    finally:
        aug.close()
