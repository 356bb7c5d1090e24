"""GPU tier of the baseline JPEG input frames (tests/jpeg_cases.py): k_jpeg_idct + k_jpeg_bgr against the numpy statement.  The
pre-pass is fed a coefficient record (RR_IN_BG_JPEG) -- laid out by the numpy parser, not by the library's reader -- and its fog layer
and environment map must equal, bit for bit, those of the same call fed the numpy-decoded pixels as RR_IN_BG_U8: a comparison that
sees one sample off by one (the way tests/test_gpu_pngrows_cases.py compares).  Refused kinds of files are the CPU tier's."""
import importlib
import os

import numpy as np
import pytest
from PIL import Image

import helpers as h
import jpeg_cases as jc
import test_gpu_prepass as tp
from oracle import prepass as op

pytestmark = pytest.mark.gpu

hb = h.hb
envmod = importlib.import_module('rain-rendering_amd.common.envmap')
fogmod = importlib.import_module('rain-rendering_amd.common.add_attenuation')
RAIN = 25


@pytest.fixture(scope="module")
def ctx(built):
    rh = hb.RainHip(0)
    rh.set_prepass_kernels(op.gaussian_kernel(25, 25), op.gaussian_kernel(15, 0))
    consts = fogmod.FogRain(rain_intensity=RAIN, focal=0.006, f_number=6.0, angle=90, exposure=2, camera_gain=20).constants()
    yield rh, consts
    rh.close()


def _record(b):
    """(record bytes on an 8-byte boundary, B G R pixels): both from the numpy statement."""
    parts = jc.coefficients(b)
    rec = jc.record_of(*parts)
    out = np.zeros(rec.size // 8, np.int64).view(np.uint8)
    out[:] = rec
    return out, jc.pixels_of(*parts)


def _depth(H, W, seed):
    return np.random.RandomState(seed).randint(256, 65536, (H, W)).astype(np.uint16)


def _geometry(rh, H, W):
    if W < 2:
        return False                                       # (the map's projection tables need a width: fog layer only)
    rh.set_envmap_geometry(H, W, *envmod.EnvironmentMapGenerator(0.006, W, H).device_tables(H, W))
    return True


def _same(got, want, what):
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs first at %s" % (what, k, np.argwhere(a != b)[:4].tolist())


@pytest.mark.parametrize("name", [c[0] for c in jc.kinds()])
def test_every_accepted_kind_gives_the_numpy_pixels(ctx, name):
    rh, consts = ctx
    _, W, H, ss, b = [c for c in jc.kinds() if c[0] == name][0]
    rec, bgr = _record(b)
    assert rec.size == hb.jpeg_record_bytes(W, H, ss) and bgr.shape == (H, W, 3)
    d16 = _depth(H, W, 1)
    env = _geometry(rh, H, W)
    want = rh.prepass_frames([dict(bg_u8=bgr, depth=d16, fog=consts)], want_env=env)[0]
    assert want['rainy_bg'].std() > 0 or H * W < 4
    got = rh.prepass_frames([dict(bg_jpeg=rec, shape=(H, W), depth_png_rows=hb.png_rows_of(d16), fog=consts)], want_env=env)[0]     # RR_DEPTH_PNG_ROWS
    _same(got, want, name + ' (depth scanlines)')
    metres = (d16.astype(np.float32) / np.float32(256.))
    got = rh.prepass_frames([dict(bg_jpeg=rec, shape=(H, W), depth=metres, fog=consts)], want_env=env)[0]                         # float depth
    _same(got, rh.prepass_frames([dict(bg_u8=bgr, depth=metres, fog=consts)], want_env=env)[0], name + ' (float depth)')


def test_three_different_images_in_one_batch_and_the_launches(ctx):
    """n = 3: the per-frame strides of records, planes and pixels; one launch of each kernel, none of the PNG un-filter; a PNG batch
    launches neither."""
    rh, consts = ctx
    W, H = 37, 29
    _geometry(rh, H, W)
    files = [jc.encode(jc.source_image(W, H, seed=s), q, jc.S420) for s, q in ((11, 50), (12, 92), (13, 100))]
    recs = [_record(b) for b in files]
    assert len({r[1].tobytes() for r in recs}) == 3
    depth = [_depth(H, W, 20 + k).astype(np.float32) / np.float32(256.) for k in range(3)]
    rh.profile(True)
    rh.profile_reset()
    got = rh.prepass_frames([dict(bg_jpeg=r[0], shape=(H, W), depth=d, fog=consts) for r, d in zip(recs, depth)])
    prof = rh.profile_read()
    rh.profile_reset()
    want = rh.prepass_frames([dict(bg_u8=r[1], depth=d, fog=consts) for r, d in zip(recs, depth)])
    prof_u8 = rh.profile_read()
    rh.profile_reset()
    rows = rh.prepass_frames([dict(bg_png_rows=hb.png_rows_of(r[1]), shape=(H, W), depth=d, fog=consts) for r, d in zip(recs, depth)])
    prof_png = rh.profile_read()
    rh.profile(False)
    assert prof.get('k_jpeg_idct', (0,))[0] == 1 and prof.get('k_jpeg_bgr', (0,))[0] == 1 and 'k_png_unfilter' not in prof, prof
    assert prof_png.get('k_png_unfilter', (0,))[0] == 1 and 'k_jpeg_idct' not in prof_png and 'k_jpeg_bgr' not in prof_png, prof_png
    assert 'k_jpeg_idct' not in prof_u8 and 'k_jpeg_bgr' not in prof_u8
    # everything else a JPEG batch launches is what the byte batch launches
    assert {k: v[0] for k, v in prof.items() if not k.startswith('k_jpeg')} == {k: v[0] for k, v in prof_u8.items()}
    for i in range(3):
        _same(got[i], want[i], 'frame %d of 3' % i)
        _same(rows[i], want[i], 'PNG frame %d of 3' % i)
        alone = rh.prepass_frames([dict(bg_jpeg=recs[i][0], shape=(H, W), depth=depth[i], fog=consts)])[0]
        _same(alone, want[i], 'frame %d alone' % i)


def test_refusals_each_followed_by_a_good_call(ctx):
    rh, consts = ctx
    W, H = 37, 29
    _geometry(rh, H, W)
    rec, bgr = _record(jc.encode(jc.source_image(W, H), 92, jc.S420))
    rec422 = _record(jc.encode(jc.source_image(W, H), 92, jc.S422))[0]
    rec_other = _record(jc.encode(jc.source_image(33, 40), 92, jc.S420))[0]
    d = _depth(H, W, 3).astype(np.float32) / np.float32(256.)
    good = dict(bg_jpeg=rec, shape=(H, W), depth=d, fog=consts)
    want = rh.prepass_frames([dict(bg_u8=bgr, depth=d, fog=consts)])[0]

    def ok():
        _same(rh.prepass_frames([good, good])[1], want, 'the good call')
    ok()
    bad_magic = rec.copy()
    bad_magic[0] ^= 1
    for what, frames in (('a mixed batch', [good, dict(bg_u8=bgr, depth=d, fog=consts)]),
                         ('a mixed batch, bytes first', [dict(bg_u8=bgr, depth=d, fog=consts), good]),
                         ('a record of another size', [good, dict(good, bg_jpeg=rec_other)]),
                         ('a record of another sampling', [good, dict(good, bg_jpeg=rec422)]),
                         ('a record without the magic word', [dict(good, bg_jpeg=bad_magic)])):
        with pytest.raises(RuntimeError):
            rh.prepass_frames(frames)
        ok()
    rh.set_input_resize(H, W, H, W)                          # armed: JPEG at a render scale other than 1 is not this route's
    try:
        with pytest.raises(RuntimeError, match='rr_set_input_resize'):
            rh.prepass_frames([dict(good, render_shape=(H // 2, W // 2), depth_shape=(H, W))])
    finally:
        rh.set_input_resize()
    ok()


def test_three_slots_in_flight(tmp_path, built):
    """Three JPEG batches in flight at once (each slot its own record and plane block) against rr_pipeline_frames on the numpy pixels."""
    H, W = 96, 160
    sc = h.Scene(tmp_path, H, W, 150, n_frames=3, seed0=31)
    rh = hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        consts, We = tp._setup(rh, H, W, 25)
        frames_j, frames_u = [], []
        for i in range(3):
            bg, depth = tp._scene(H, W, 31 + i)
            rec, bgr = _record(jc.encode(np.ascontiguousarray((bg[..., ::-1] * 255).astype(np.uint8)), 92, (jc.S420, jc.S420, jc.S444)[i]))
            pinned = rh.host_array((rec.size,), np.uint8)
            pinned[...] = rec
            dep = rh.host_array((H, W), np.float32)
            dep[...] = depth.astype(np.float32)
            common = dict(depth=dep, fog=consts, omega=sc.omega, drops=sc.product_drops(i))
            frames_j.append(dict(common, bg_jpeg=pinned, shape=(H, W)))
            frames_u.append(dict(common, bg_u8=bgr))
        ref = rh.pipeline_frames(frames_u, want_mask_i32=True)
        outs = [dict(image_u8=rh.host_array((H, W, 3), np.uint8), mask_i32=rh.host_array((H, W), np.int32),
                     status=np.zeros(len(frames_j[i]['drops']), np.int32)) for i in range(3)]
        for slot in range(3):
            rh.pipeline_submit(slot, frames_j[slot:slot + 1], outs[slot:slot + 1])
        for slot in range(3):
            assert rh.pipeline_wait(slot)
        for i, (o, r) in enumerate(zip(outs, ref)):
            for k in ('image_u8', 'mask_i32', 'status'):
                assert np.array_equal(o[k], r[k]), (i, k)
        assert ref[0]['mask_i32'].any()
    finally:
        rh.close()


def _tree(tmp, name, n, H, W, as_jpeg):
    """The synthetic kitti tree; as_jpeg: its images as .jpg / .jpeg files, else as PNG files holding PIL's decode of those."""
    src = os.path.join(tmp, name)
    img_dir, _ = h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), n, H, W, depth_m=None)
    for i in range(n):
        png = os.path.join(img_dir, '%06d.png' % i)
        b = jc.encode(np.array(Image.open(png).convert('RGB')), 92, jc.S420, optimize=bool(i & 1))
        if as_jpeg:
            os.remove(png)
            with open(os.path.join(img_dir, '%06d%s' % (i, '.jpeg' if i & 1 else '.jpg')), 'wb') as f:
                f.write(b)
        else:
            Image.fromarray(np.ascontiguousarray(jc.pil_bgr(b)[..., ::-1])).save(png)
    return src


@pytest.mark.parametrize("extra", [(), ('--rain_layer',)])
def test_main_device_particles_on_a_jpeg_tree_writes_the_png_trees_files(tmp_path, built, monkeypatch, extra):
    tmp = str(tmp_path)
    H, W, n = 375, 1242, 3                                             # KITTI's frames: the device's particle generator renders the sensor's size
    h.synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
    monkeypatch.setenv('RAIN_BATCH', '2')                              # two batches, the second ragged
    main = importlib.import_module('rain-rendering_amd.main')
    outs = {}
    for kind in ('jpeg', 'png'):
        src = _tree(tmp, 'source_' + kind, n, H, W, kind == 'jpeg')
        gen = main.main(['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', os.path.join(tmp, 'rainstreakdb'),
                         '-i', '5', '--output', os.path.join(tmp, 'out_' + kind), '--noverbose', '--device_particles'] + list(extra))
        assert gen.timing[0].get('route') == 'native' and len(gen.stats) == n and all(s['drops'] > 20 for s in gen.stats)
        outs[kind] = os.path.join(tmp, 'out_' + kind, 'kitti', 'data_object', 'training', 'rain', '5mm')
    for folder in ('rainy_image', 'rain_mask') + (('rain_layer',) if extra else ()):
        names = sorted(os.listdir(os.path.join(outs['png'], folder)))
        assert names == ['%06d.png' % i for i in range(n)] == sorted(os.listdir(os.path.join(outs['jpeg'], folder))), folder
        for nm in names:
            a, b = (open(os.path.join(outs[k], folder, nm), 'rb').read() for k in ('jpeg', 'png'))
            assert a == b, (folder, nm)
    first = np.array(Image.open(os.path.join(outs['jpeg'], 'rain_mask', '000000.png')))
    assert first[..., :3].std() > 0                                    # (there is rain in the files)
