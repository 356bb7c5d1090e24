"""GPU tier of RainAugment (rain-rendering_amd/augment.py, rr_augment_frames_device): the same pixels as the driver's files and
as rr_pipeline_frames fed the same records, mixed intensities, the caller's stream, odd frame sizes, determinism."""
import importlib
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

import helpers as h

pytestmark = pytest.mark.gpu

augment = importlib.import_module('rain-rendering_amd.augment')
dbmod = importlib.import_module('rain-rendering_amd.common.db')
imgops = importlib.import_module('rain-rendering_amd.common.imgops')
envmod = importlib.import_module('rain-rendering_amd.common.envmap')

DEV = torch.device('cuda', 0)


@pytest.fixture(scope='module')
def streaks_db(tmp_path_factory):
    root = os.path.join(str(tmp_path_factory.mktemp('augdb')), 'rainstreakdb')
    h.synthetic.write_streak_db(root)
    return root


def _scene(n, H, W, seed=0):
    """n planar RGB byte images [n, 3, H, W] and their BGR / depth arrays (a depth ramp: the fog layer varies by row)."""
    bgr = np.stack([(h.synthetic.make_frame(seed + i, H, W) * 255).astype(np.uint8) for i in range(n)])
    depth = np.stack([(np.linspace(80.0, 2.0, H)[:, None] * np.ones((1, W))).astype(np.float32) + i for i in range(n)])
    return bgr, depth


def _planar(bgr):
    return torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)))


def _pipeline(aug, p, bgr, depth):
    """rr_pipeline_submit on the same records, inputs as interleaved BGR (bytes, or float32 -> RR_IN_BG_F32), the default
    hand-over (float32, resident solid angles): [(image_u8 RGB, mask_f64)] per frame."""
    n, H, W = bgr.shape[:3]
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(aug.db.streaks_light)
        rh.set_camera(h.hb.make_camera(aug.focal, aug.f_number, aug.exposure))
        rh.set_prepass_kernels(imgops.gaussian_kernel(25, 25), imgops.gaussian_kernel(15, 0))
        rh.set_particle_tables(p['d_grid'], p['cdf'])
        we = rh.set_envmap_geometry(H, W, *envmod.EnvironmentMapGenerator(aug.focal, W, H).device_tables(H, W))
        rh.set_solid_angles(h.solid_angle.get_solid_angles(np.empty((H, we, 0))))
        frames, outs = [], []
        for i in range(n):
            img = dict(bg_u8=np.ascontiguousarray(bgr[i])) if bgr.dtype == np.uint8 else dict(bg=np.ascontiguousarray(bgr[i]))
            frames.append(dict(img, depth=np.ascontiguousarray(depth[i]), fog=tuple(p['fog'][i]), omega=None,
                               sim=p['sims'][i:i + 1].copy(), drops_cap=p['drops_cap']))
            outs.append(dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W))))
        rh.pipeline_submit(0, frames, outs)
        while not rh.pipeline_wait(0):
            rh.pipeline_submit(0, frames, outs)
    finally:
        rh.close()
    return [(o['image_u8'], o['mask']) for o in outs]


def _check_against_pipeline(aug, bgr8, depth, rate, idx):
    """Bytes and float32 inputs through RainAugment and through rr_pipeline_frames on the same records."""
    p = aug.plan(rate, idx)
    d = torch.from_numpy(depth).to(DEV)
    rainy8, mask8 = aug(_planar(bgr8).to(DEV), d, rate, idx)
    f32 = (bgr8.astype(np.float64) / 255.0).astype(np.float32)
    rainyf, maskf = aug(_planar(f32).to(DEV), d[:, None], rate, idx)
    assert rainy8.dtype == torch.uint8 and rainyf.dtype == torch.float32 and mask8.shape == (len(idx), 1) + bgr8.shape[1:3]
    rainy8, mask8, rainyf, maskf = (t.cpu().numpy() for t in (rainy8, mask8, rainyf, maskf))
    for img_in, rainy, mask in ((bgr8, rainy8, mask8), (f32, rainyf, maskf)):
        ref = _pipeline(aug, p, img_in, depth)
        for i, (img_u8, m64) in enumerate(ref):
            got = rainy[i].transpose(1, 2, 0)
            if rainy.dtype == np.uint8:
                assert np.array_equal(got, img_u8), i
            else:
                assert np.array_equal(got, img_u8.astype(np.float32) / np.float32(255.0)), i
            assert np.array_equal(mask[i, 0], m64.astype(np.float32)), i
            assert m64.max() > 0, i                                     # streaks were rendered


def test_same_pixels_as_the_driver_files(tmp_path, built, streaks_db):
    tmp = str(tmp_path)
    H, W, n = 375, 1242, 3
    src = os.path.join(tmp, 'source')
    h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), n, H, W, depth_m=None)
    main = importlib.import_module('rain-rendering_amd.main')
    gen = main.main(['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', streaks_db,
                     '-i', '25', '--output', os.path.join(tmp, 'out'), '--noverbose', '--device_particles'])
    assert len(gen.stats) == n
    img_dir = os.path.join(src, 'kitti', 'data_object', 'training', 'image_2')
    rgb = np.stack([np.array(Image.open(os.path.join(img_dir, '%06d.png' % i)).convert('RGB')) for i in range(n)])
    depth = np.stack([np.array(Image.open(os.path.join(img_dir, 'depth', '%06d.png' % i))).astype(np.float32) / 256. for i in range(n)])
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training')
    try:
        rainy, mask = aug(torch.from_numpy(rgb.transpose(0, 3, 1, 2).copy()).to(DEV), torch.from_numpy(depth).to(DEV), 25, list(range(n)))
        rainy = rainy.cpu().numpy()
        out_dir = os.path.join(tmp, 'out', 'kitti', 'data_object', 'training', 'rain', '25mm', 'rainy_image')
        for i in range(n):
            got = np.array(Image.open(os.path.join(out_dir, '%06d.png' % i)))[..., :3]
            assert np.array_equal(rainy[i].transpose(1, 2, 0), got), i
            assert not np.array_equal(got, rgb[i]) and float(mask[i].max()) > 0, i
    finally:
        aug.close()


@pytest.mark.parametrize('dataset, seq', [('kitti', 'data_object/training'), ('nuscenes', None)])
def test_same_bits_as_rr_pipeline_frames(built, streaks_db, dataset, seq):
    aug = augment.RainAugment(dataset, streaks_db=streaks_db, sequence=seq)
    try:
        H, W = aug.frame_size()
        bgr, depth = _scene(2, H, W, seed=40)
        _check_against_pipeline(aug, bgr, depth, 25, [4, 11])
    finally:
        aug.close()


def test_mixed_intensities_equal_single_intensity_calls(built, streaks_db):
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training')
    try:
        H, W = aug.frame_size()
        bgr, depth = _scene(3, H, W, seed=7)
        img, dep = _planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV)
        rates, idx = [5, 25, 100], [2, 3, 4]
        rainy, mask = aug(img, dep, rates, idx)
        for i in range(3):
            r1, m1 = aug(img[i:i + 1], dep[i:i + 1], rates[i], [idx[i]])
            assert torch.equal(rainy[i:i + 1], r1) and torch.equal(mask[i:i + 1], m1), rates[i]
        assert len({float(mask[i].sum()) for i in range(3)}) == 3          # three different rains
    finally:
        aug.close()


def test_callers_stream_and_odd_frame_sizes(built, streaks_db, monkeypatch):
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training')
    try:
        H, W = aug.frame_size()
        bgr, depth = _scene(3, H, W, seed=3)
        src, dsrc = _planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV)
        ref = aug(src, dsrc, 25, [5, 6, 7])
        torch.cuda.synchronize()
        s = torch.cuda.Stream(DEV)
        with torch.cuda.stream(s):
            # inputs made by torch kernels on s right before the call, no synchronisation in between
            img = torch.flip(torch.flip(src, [3]), [3])
            dep = dsrc * 1.0
            got = aug(img, dep, 25, [5, 6, 7])
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    finally:
        aug.close()
    # a camera with an odd width and H * W = 3 (mod 4): every plane of the batch starts on another byte boundary
    odd = types.SimpleNamespace(settings=lambda: {
        "cam_CCD_WH": [641, 359], "cam_WH": [641, 359], "cam_focal": 6, "cam_gain": 20, "cam_f_number": 6.0,
        "cam_focus_plane": 6.0, "cam_exposure": 2, "cam_pos": [1.5, 1.5, 0.3], "cam_lookat": [1.5, 1.5, -1.],
        "cam_up": [0., 1., 0.], "sequences": {}})
    monkeypatch.setitem(dbmod.dbs, 'oddcam', odd)
    aug = augment.RainAugment('oddcam', streaks_db=streaks_db)
    try:
        assert aug.frame_size() == (359, 641) and (359 * 641) % 4 == 3
        bgr, depth = _scene(3, 359, 641, seed=11)
        _check_against_pipeline(aug, bgr, depth, 50, [0, 1, 9])
    finally:
        aug.close()


def test_deterministic_and_seeded(built, streaks_db):
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training')
    aug1 = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', seed=1)
    try:
        H, W = aug.frame_size()
        bgr, depth = _scene(2, H, W, seed=21)
        img, dep = _planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV)
        a = aug(img, dep, 25, [10, 20])
        b = aug(img, dep, 25, [10, 20])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c = aug(img, dep, 25, [11, 20])
        assert not torch.equal(a[1][0], c[1][0]) and torch.equal(a[1][1], c[1][1])
        d = aug1(img, dep, 25, [10, 20])
        assert not torch.equal(a[1][0], d[1][0]) and not torch.equal(a[1][1], d[1][1])
    finally:
        aug.close()
        aug1.close()
