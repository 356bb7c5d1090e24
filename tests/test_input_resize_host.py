"""CPU tier of the render-scale resize of the inputs.  csrc/rr_resize.h is the one statement of the resize: its g++
build (tests/hostemu/resize_emu.cpp -- the loops the kernels k_resize_in / k_resize_depth run per output sample) equals
common/imgops.py resize_linear for every case and kind of tests/resize_cases.py, and rr_io_read_frames_scaled, which calls the
same header, still returns the arrays it did.  Then the driver with --device_resize around a recording stand-in context, and
RainAugment(source_size=)'s plan and shape checks.  Bit for bit throughout: + - * / floor in IEEE float64, one rounding for depth."""
import ctypes
import importlib
import os

import numpy as np
import pytest
from PIL import Image

import helpers as h
import resize_cases as rc

hb = h.hb
imgops = rc.imgops
KIND_CODE = {'bgr_u8': hb.RR_RESIZE_BGR_U8, 'rgb_u8_planar': hb.RR_RESIZE_RGB_U8_PLANAR, 'rgb_f32_planar_bytes': hb.RR_RESIZE_RGB_F32_PLANAR,
             'rgb_f32_planar': hb.RR_RESIZE_RGB_F32_PLANAR}


@pytest.fixture(scope="module")
def emu(built):
    return ctypes.CDLL(importlib.import_module('__graft_entry__').build_emu('resizeemu'))


def _where(a, b):
    return np.argwhere(a != b)[:4].tolist()


@pytest.mark.parametrize("kind", rc.IMAGE_KINDS)
@pytest.mark.parametrize("case", sorted(rc.IMAGE_CASES))
def test_header_image_equals_resize_linear(emu, case, kind):
    (H, W), (sH, sW) = rc.IMAGE_CASES[case]
    arr, _, _ = rc.image_input(case, kind)
    want = rc.image_want(case, kind)
    for f in range(rc.N):
        src = np.ascontiguousarray(arr[f])
        out = np.full((H, W, 3), np.nan)
        assert emu.resize_emu_image(h._p(src), KIND_CODE[kind], sH, sW, H, W, h._p(out)) == 0
        assert np.array_equal(out, want[f]), (case, kind, f, _where(out, want[f]))
    assert want.std() > 0 and (case == 'd' or not np.array_equal(want[2], want[1]))


@pytest.mark.parametrize("kind", rc.DEPTH_KINDS)
@pytest.mark.parametrize("case", sorted(rc.DEPTH_CASES))
def test_header_depth_equals_resize_linear(emu, case, kind):
    (H, W), (sH, sW) = rc.DEPTH_CASES[case]
    arr = rc.depth_input(case, kind)
    want = rc.depth_want(case, kind)
    for f in range(rc.N):
        src = np.ascontiguousarray(arr[f])
        out = np.full((H, W), np.nan, np.float32)
        assert emu.resize_emu_depth(h._p(src), hb.RR_DEPTH_U16 if kind == 'u16' else 0, sH, sW, H, W, h._p(out)) == 0
        assert np.array_equal(out, want[f]), (case, kind, f, _where(out, want[f]))
    assert want.dtype == np.float32 and want.std() > 0


def test_coordinates_at_the_edges(emu):
    """What the cases are chosen for, on resize_linear's own tables: up-sampling has floor(f) < 0 at index 0 (weight 0, index clamped)
    and the second index clamped at s - 1; scale 2 has every weight 0.5; the fractional case has weights that differ."""
    def coords(d, s):
        f = (np.arange(d) + 0.5) * (s / d) - 0.5
        i0 = np.floor(f).astype(np.int64)
        return i0, f - i0
    i0, w = coords(80, 40)
    assert i0[0] == -1 and i0[-1] + 1 == 40
    assert set(coords(80, 160)[1]) == {0.5} and len(set(coords(80, 161)[1])) > 40 and len(set(coords(48, 97)[1])) > 24


@pytest.mark.parametrize("image_case,depth_case", [('a', 'f'), ('b', 'g'), ('a', 'e')])
def test_host_loader_still_returns_the_same_arrays(built, tmp_path, image_case, depth_case):
    """rr_io_read_frames_scaled (now on csrc/rr_resize.h) on PNG files of the cases: image / 255 and metres resized as resize_linear
    does.  The render scale is the image case's; the depth scale is what makes the depth file's scaled size the frame's."""
    (H, W), (sH, sW) = rc.IMAGE_CASES[image_case]
    (dHo, dWo), (dH, dW) = rc.DEPTH_CASES[depth_case]
    assert (dHo, dWo) == (H, W)
    rs = sH // H
    ds = {'e': 4, 'f': 1, 'g': 1}[depth_case]
    assert (sH // rs, sW // rs) == (H, W) and ((dH * ds) // rs, (dW * ds) // rs) == (H, W)
    bgr, d16 = rc.image_bytes(image_case), rc.depth_input(depth_case, 'u16')
    ips, dps = [], []
    for f in range(rc.N):
        ips.append(str(tmp_path / ('i%d.png' % f)))
        dps.append(str(tmp_path / ('d%d.png' % f)))
        Image.fromarray(np.ascontiguousarray(bgr[f][..., ::-1])).save(ips[-1])
        Image.fromarray(d16[f]).save(dps[-1])
    bg = np.zeros((rc.N, H * W * 24), np.uint8)
    dep = np.zeros((rc.N, H * W * 4), np.uint8)
    st = hb.io_read_frames_scaled(ips, dps, H, W, rs, ds, bg, dep, 2)
    assert not np.any(st), st
    assert np.array_equal(bg.view(np.float64).reshape(rc.N, H, W, 3), rc.image_want(image_case, 'bgr_u8'))
    assert np.array_equal(dep.view(np.float32).reshape(rc.N, H, W), rc.depth_want(depth_case, 'u16'))


# ---- the driver with --device_resize around a recording stand-in context ---------------------------------------------------------
import test_driver_host as tdh                                       # noqa: E402  (the stand-in context and the dataset maker)
import test_pngrows_host as tph                                      # noqa: E402  (the host build of the device's un-filter rule)

RH, RW = 48, 80                                                      # render size of the driver tests: 96 x 160 files at render_scale 2


def _host_stage(fr):
    """What the armed library makes of a frame's source-size scanlines, on the host: un-filter, then resize_linear."""
    (sh, sw), (dh, dw), (H, W) = fr['shape'], fr['depth_shape'], fr['render_shape']
    bgr = tph._unfilter(np.ascontiguousarray(fr['bg_png_rows']), sh, sw, 3)
    d16 = tph._unfilter(np.ascontiguousarray(fr['depth_png_rows']), dh, dw, 2)
    depth = d16.astype(np.float32) / np.float32(256.)
    return dict(fr, bg=imgops.resize_linear(bgr / 255.0, W, H), bg_u8=None, bg_png_rows=None, depth_png_rows=None,
                depth=depth if (dh, dw) == (H, W) else imgops.resize_linear(depth, W, H).astype(np.float32))


class ResizeRecordingContext(tdh.RecordingContext):
    """Records set_input_resize and the shapes of the rows it is handed; logs and "renders" every frame as the arrays the armed
    library would make of it."""
    calls, shapes = None, None

    def set_input_resize(self, *sizes):
        ResizeRecordingContext.calls.append(tuple(int(v) for v in sizes))

    def pipeline_submit_prepared(self, slot, prep, n=None):
        if any(fr.get('render_shape') is not None for fr in prep.frames) or hasattr(prep, 'src_frames'):
            if not hasattr(prep, 'src_frames'):
                prep.src_frames = prep.frames
            for fr in prep.src_frames[:prep.n if n is None else n]:
                ResizeRecordingContext.shapes.add((fr['shape'], np.asarray(fr['bg_png_rows']).size, fr['depth_shape'],
                                                   np.asarray(fr['depth_png_rows']).size, fr['render_shape']))
            prep.frames = [_host_stage(fr) for fr in prep.src_frames]
        super().pipeline_submit_prepared(slot, prep, n)


def _driver_run(tmp, src, out_name, monkeypatch, flags, batch=2):
    monkeypatch.setenv('RAIN_BATCH', str(batch))
    monkeypatch.setenv('RAIN_NATIVE_IO', '1')
    monkeypatch.setattr(hb, 'RainHip', ResizeRecordingContext)
    tdh.RecordingContext.log = []
    ResizeRecordingContext.calls, ResizeRecordingContext.shapes = [], set()
    argv = ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', os.path.join(tmp, 'rainstreakdb'),
            '-i', '5', '--output', os.path.join(tmp, out_name), '--noverbose'] + flags
    gen = tdh.main_mod.main(argv)
    return gen, tdh.RecordingContext.log, list(ResizeRecordingContext.calls), set(ResizeRecordingContext.shapes)


def _scaled_settings(monkeypatch, render_scale, depth_scale):
    kitti = importlib.import_module('rain-rendering_amd.config.kitti')
    plain = kitti.settings

    def scaled():
        st = dict(plain())
        st["render_scale"], st["depth_scale"] = render_scale, depth_scale
        return st
    monkeypatch.setattr(kitti, 'settings', scaled)


def _small_depth(dep_dir, n, dh, dw):
    """Depth files of another size than the images: noise between 2 and 80 m."""
    for i in range(n):
        d = np.random.RandomState(900 + i).randint(512, 20480, (dh, dw)).astype(np.uint16)
        Image.fromarray(d).save(os.path.join(dep_dir, '%06d.png' % i))


def test_driver_arms_the_stage_and_hands_over_source_size_rows(tmp_path, built, monkeypatch):
    tmp = str(tmp_path)
    n = 5
    src, img_dir, dep_dir = tdh._dataset(tmp, n, H=96, W=160)
    _small_depth(dep_dir, n, RH, RW)
    _scaled_settings(monkeypatch, 2, 2)
    gen_d, log_d, calls_d, shapes_d = _driver_run(tmp, src, 'out_default', monkeypatch, [])
    gen_r, log_r, calls_r, shapes_r = _driver_run(tmp, src, 'out_resize', monkeypatch, ['--device_resize'])
    assert gen_d.timing[0].get('route') == 'native' and gen_r.timing[0].get('route') == 'native'
    assert calls_d == [] and shapes_d == set()                           # without the flag nothing is armed
    assert calls_r == [(96, 160, RH, RW)]                                # armed once for the run
    assert shapes_r == {((96, 160), 96 * (1 + 3 * 160), (RH, RW), RH * (1 + 2 * RW), (RH, RW))}
    assert len(log_d) == len(log_r) == n
    a = {fr['bg'].tobytes(): fr for fr in log_d}
    b = {fr['bg'].tobytes(): fr for fr in log_r}
    assert a.keys() == b.keys() and len(a) == n                          # the same float64 images, bit for bit
    for key in a:
        assert a[key]['bg'].dtype == b[key]['bg'].dtype == np.float64 and a[key]['bg'].shape == (RH, RW, 3)
        assert b[key]['depth'].dtype == np.float32 and np.array_equal(a[key]['depth'], b[key]['depth'])
        assert len(a[key]['drops']) > 10 and a[key]['drops'].tobytes() == b[key]['drops'].tobytes()
    for i in range(n):
        assert np.array(Image.open(os.path.join(tmp, 'out_resize', 'kitti', 'data_object', 'training', 'rain', '5mm', 'rainy_image',
                                                '%06d.png' % i))).shape == (RH, RW, 4)


def test_driver_resizes_a_full_size_depth_map_and_falls_back_per_frame(tmp_path, built, monkeypatch):
    """Depth files of the images' size (depth_scale 1) are resized by the stage too; a frame the fast reader refuses (a palette
    image here) arrives as rows of filter type 0 at the source size; without a resize to do the flag is a no-op."""
    tmp = str(tmp_path)
    n = 4
    src, img_dir, dep_dir = tdh._dataset(tmp, n, H=96, W=160)
    _small_depth(dep_dir, n, 96, 160)
    Image.open(os.path.join(img_dir, '%06d.png' % 1)).convert('RGB').quantize(64).save(os.path.join(img_dir, '%06d.png' % 1))
    _scaled_settings(monkeypatch, 2, 1)
    gen_d, log_d, calls_d, _ = _driver_run(tmp, src, 'out_default', monkeypatch, [])
    gen_r, log_r, calls_r, shapes_r = _driver_run(tmp, src, 'out_resize', monkeypatch, ['--device_resize'])
    assert calls_d == [] and calls_r == [(96, 160, 96, 160)] and len(shapes_r) == 1
    a = {fr['bg'].tobytes(): fr for fr in log_d}
    b = {fr['bg'].tobytes(): fr for fr in log_r}
    assert a.keys() == b.keys() and len(a) == n
    for key in a:
        assert np.array_equal(a[key]['depth'], b[key]['depth']) and a[key]['depth'].shape == (RH, RW)
    _scaled_settings(monkeypatch, 1, 1)                                  # nothing to resize: the default route, nothing armed
    gen_p, log_p, calls_p, shapes_p = _driver_run(tmp, src, 'out_plain', monkeypatch, ['--device_resize'])
    assert gen_p.timing[0].get('route') == 'native' and calls_p == [] and shapes_p == set() and len(log_p) == n


# ---- RainAugment(source_size=, depth_size=): plan and shape checks ----------------------------------------------------------------
def test_augment_source_size_plan_and_validation(tmp_path):
    import torch
    augment = importlib.import_module('rain-rendering_amd.augment')
    h.synthetic.write_streak_db(os.path.join(str(tmp_path), 'rainstreakdb'))
    db = os.path.join(str(tmp_path), 'rainstreakdb')
    plain = augment.RainAugment('kitti', streaks_db=db, sequence='data_object/training')
    fh, fw = plain.frame_size()
    assert plain.source_size is None and plain.depth_size is None and plain.plan(25, [0])['source_size'] is None
    assert augment.RainAugment('kitti', streaks_db=db, depth_size=(fh, fw)).source_size is None       # the render size: nothing to do
    with pytest.raises(ValueError, match='source_size'):
        augment.RainAugment('kitti', streaks_db=db, depth_size=(fh // 2, fw // 2))
    for bad in ((0, 10), (10,), 'ab', (10.5, 3), (16385, 4), (True, 4)):
        with pytest.raises(ValueError, match='source_size'):
            augment.RainAugment('kitti', streaks_db=db, source_size=bad)
    aug = augment.RainAugment('kitti', streaks_db=db, sequence='data_object/training', source_size=(2 * fh, 2 * fw + 1))
    assert aug.frame_size() == (fh, fw) and aug.source_size == (2 * fh, 2 * fw + 1) and aug.depth_size == (fh, fw)
    p, q = aug.plan(25, [3, 4]), plain.plan(25, [3, 4])
    assert p['source_size'] == (2 * fh, 2 * fw + 1) and p['depth_size'] == (fh, fw) and p['frame_size'] == (fh, fw)
    assert p['sims'].tobytes() == q['sims'].tobytes() and np.array_equal(p['fog'], q['fog']) and p['drops_cap'] == q['drops_cap']
    aug2 = augment.RainAugment('kitti', streaks_db=db, source_size=(2 * fh, 2 * fw), depth_size=(fh // 2, fw // 2))
    assert aug2.depth_size == (fh // 2, fw // 2)
    img = torch.zeros((2, 3, 2 * fh, 2 * fw + 1), dtype=torch.uint8)
    assert aug._validate(img, torch.zeros((2, fh, fw))) == (2, 2 * fh, 2 * fw + 1)
    assert aug._validate(img, torch.zeros((2, 1, fh, fw)))[0] == 2
    with pytest.raises(ValueError, match='depth must be'):               # depth at the source size, not at depth_size
        aug._validate(img, torch.zeros((2, 2 * fh, 2 * fw + 1)))
    with pytest.raises(ValueError, match='source_size'):                 # images at the render size
        aug(torch.zeros((2, 3, fh, fw), dtype=torch.uint8), torch.zeros((2, fh, fw)), 25, [0, 1])
    with pytest.raises(ValueError, match='depth must be'):
        aug2._validate(torch.zeros((1, 3, 2 * fh, 2 * fw), dtype=torch.uint8), torch.zeros((1, fh, fw)))
