"""GPU tier of the tensor formats of RainAugment / rr_augment_frames_device: float16 and bfloat16 batches, and
channels-last (interleaved) batches of all four dtypes, in and out.  Every comparison is bit for bit:

  1. halves, planar        aug(x_h) == aug(x_h.float()) rounded once to the half type; the same mask;
  2. interleaved           aug(x_cl) == aug(x) value for value, with x_cl's strides, x_cl untouched;
  3. the library           rr_augment_frames_device on buffers one element off a 16-byte boundary, guard bytes around the outputs;
  4. a rig                 [B, 2, 3, H, W] with NHWC inner strides;
  5. source_size=          every new format through the armed input resize;
  6. lens=                 uint8 channels-last through RR_TENSOR_U8_HWC, LensAugment likewise, the refused combinations;
  7. a side stream;        8. every RR_E_ARG, and a valid call after each.

The frames are 161 x 97: H W = 15 617 = 1 (mod 16, 8 and 4), so every lane width of the ingest and finalize kernels has a tail and the
three frames of a batch start on three different byte residues in every format.  The images carry a stripe of exact 0 and 1, a
stripe of half subnormals and a stripe of the smallest normals."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import helpers as h
import test_gpu_augment as tga

pytestmark = pytest.mark.gpu

augment = tga.augment
dbmod = tga.dbmod
hb = h.hb
lens = importlib.import_module('rain-rendering_amd.tools.lens')
rigmod = importlib.import_module('rain-rendering_amd.rig')

DEV = tga.DEV
H, W, N = 97, 161, 3
RATE, IDX = 50, [0, 1, 9]
DTYPES = [torch.uint8, torch.float32, torch.float16, torch.bfloat16]
HALVES = [torch.float16, torch.bfloat16]
CL = torch.channels_last
CODE = {torch.uint8: hb.RR_TENSOR_U8, torch.float32: hb.RR_TENSOR_F32, torch.float16: hb.RR_TENSOR_F16, torch.bfloat16: hb.RR_TENSOR_BF16}


@pytest.fixture(scope='module')
def streaks_db(tmp_path_factory):
    root = os.path.join(str(tmp_path_factory.mktemp('fmtdb')), 'rainstreakdb')
    h.synthetic.write_streak_db(root)
    return root


def _bits(t):
    """`t` as integers of its element size: a comparison of bit patterns, whatever the strides."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _stripes(x):
    """Rows 0 .. 3 exact 0 and 1, rows 4 .. 7 the type's subnormals, rows 8 .. 11 its smallest normals (a half tensor [n, 3, H, W])."""
    man = 10 if x.dtype == torch.float16 else 7
    bits = x.view(torch.int16)
    n = bits[:, :, 0:4].numel()
    k = torch.arange(n, dtype=torch.int32)
    bits[:, :, 0:4] = torch.where(k % 2 == 0, 0, 0x3c00 if x.dtype == torch.float16 else 0x3f80).to(torch.int16).reshape(bits[:, :, 0:4].shape)
    bits[:, :, 4:8] = (1 + k % ((1 << man) - 1)).to(torch.int16).reshape(bits[:, :, 4:8].shape)          # 1 .. 2^man - 1
    bits[:, :, 8:12] = ((1 << man) + k % 5).to(torch.int16).reshape(bits[:, :, 8:12].shape)
    return x


def _images(dtype, n=N, h_=H, w_=W, seed=11):
    """A seeded scene as planar [n, 3, h, w] of `dtype` on the CPU, with the stripes (bytes: 0 and 255)."""
    bgr, _ = tga._scene(n, h_, w_, seed=seed)
    if dtype == torch.uint8:
        x = tga._planar(bgr).clone()
        x[:, :, 0:4, 0::2], x[:, :, 0:4, 1::2] = 0, 255
        return x
    f32 = tga._planar((bgr.astype(np.float64) / 255.0).astype(np.float32)).clone()
    if dtype in HALVES:
        return _stripes(f32.to(dtype))
    x = f32                                              # float32: both half types' stripes (bfloat16's subnormals are float32's)
    x[:, :, 0:12, : w_ // 2] = _stripes(f32.to(torch.bfloat16)).float()[:, :, 0:12, : w_ // 2]
    x[:, :, 0:12, w_ // 2:] = _stripes(f32.to(torch.float16)).float()[:, :, 0:12, w_ // 2:]
    return x


def _depth(n=N, h_=H, w_=W, seed=11):
    return torch.from_numpy(tga._scene(n, h_, w_, seed=seed)[1])


class World:
    """One augmenter on the 161 x 97 camera and the planar results of the four dtypes, computed once and never changed."""

    def __init__(self, db):
        self.aug = augment.RainAugment('fmtcam', streaks_db=db)
        assert self.aug.frame_size() == (H, W) and (H * W) % 16 == 1
        self.depth = _depth().to(DEV)
        self.x = {dt: _images(dt).to(DEV) for dt in DTYPES}
        self.ref = {}

    def planar(self, dtype):
        if dtype not in self.ref:
            rainy, mask = self.aug(self.x[dtype], self.depth, RATE, IDX)
            assert rainy.dtype == dtype and rainy.is_contiguous() and all(float(mask[i].max()) > 0 for i in range(N))
            self.ref[dtype] = (rainy, mask)
        return self.ref[dtype]


@pytest.fixture(scope='module')
def world(built, streaks_db):
    cam = types.SimpleNamespace(settings=lambda: {
        "cam_CCD_WH": [W, H], "cam_WH": [W, H], "cam_focal": 6, "cam_gain": 20, "cam_f_number": 6.0,
        "cam_focus_plane": 6.0, "cam_exposure": 2, "cam_pos": [1.5, 1.5, 0.3], "cam_lookat": [1.5, 1.5, -1.],
        "cam_up": [0., 1., 0.], "sequences": {}})
    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(dbmod.dbs, 'fmtcam', cam)
        w = World(streaks_db)
        yield w
        w.aug.close()


# ---- 1. halves, planar ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALVES)
def test_half_batches_are_the_float32_result_rounded_once(world, dtype):
    x = world.x[dtype]
    sub = x[:, :, 4:8].cpu().float()
    assert float(sub.max()) < (2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126) and float(sub.min()) > 0          # the subnormal stripe
    rainy, mask = world.planar(dtype)
    want, want_mask = world.aug(x.float(), world.depth, RATE, IDX)
    assert rainy.dtype == dtype and want.dtype == torch.float32 and rainy.shape == x.shape
    assert torch.equal(rainy, want.to(dtype)) and torch.equal(mask, want_mask)
    assert not torch.equal(rainy, x) and torch.equal(mask, world.planar(torch.uint8)[1])
    one, one_mask = world.aug(x[:1], world.depth[:1], RATE, IDX[:1])                                          # one frame
    assert torch.equal(one, rainy[:1]) and torch.equal(one_mask, mask[:1])


# ---- 2. interleaved, all four dtypes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_channels_last_batches_come_back_channels_last(world, dtype):
    x = world.x[dtype]
    x_cl = x.contiguous(memory_format=CL)
    keep = x_cl.clone()
    assert not x_cl.is_contiguous() and x_cl.is_contiguous(memory_format=CL)
    want, want_mask = world.planar(dtype)
    rainy, mask = world.aug(x_cl, world.depth, RATE, IDX)
    assert rainy.dtype == dtype and rainy.stride() == x_cl.stride() and rainy.is_contiguous(memory_format=CL)
    assert torch.equal(rainy, want) and torch.equal(mask, want_mask)
    assert torch.equal(_bits(x_cl), _bits(keep))                                                            # the input is never written
    one_cl = x[1:2].contiguous(memory_format=CL)                                                              # one frame
    one, one_mask = world.aug(one_cl, world.depth[1:2], RATE, IDX[1:2])
    assert one.stride() == one_cl.stride() and torch.equal(one, want[1:2]) and torch.equal(one_mask, want_mask[1:2])
    # a decoder's [B, H, W, 3] frames seen as [B, 3, H, W]
    hwc = x.permute(0, 2, 3, 1).contiguous()
    again, _ = world.aug(hwc.permute(0, 3, 1, 2), world.depth, RATE, IDX)
    assert torch.equal(again.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1)) and again.permute(0, 2, 3, 1).is_contiguous()


# ---- 3. the library, buffers one element off a 16-byte boundary, guard bands ---------------------------------------------------------------
def _carve(nbytes, off, fill):
    """(the whole byte tensor, its slice [off, off + nbytes)): the slice starts `off` bytes behind a 16-byte boundary."""
    buf = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + nbytes]


def _frames_bytes(t, interleaved):
    """The bytes of [n, 3, H, W] `t` as the library's layout holds them."""
    t = t.permute(0, 2, 3, 1).contiguous() if interleaved else t.contiguous()
    return t.reshape(-1).view(torch.uint8)


# the eight formats on three frames, and one of them on one frame
LIB_CASES = [(dt, il, N) for dt in DTYPES for il in (False, True)] + [(torch.bfloat16, True, 1)]


@pytest.mark.parametrize("dtype, interleaved, n", LIB_CASES, ids=lambda v: str(v))
def test_library_call_with_offset_buffers_and_guard_bands(world, dtype, interleaved, n):
    want, want_mask = world.planar(dtype)
    want, want_mask = want[:n], want_mask[:n]
    el = world.x[dtype].element_size()
    src = _frames_bytes(world.x[dtype][:n], interleaved)
    nb = src.numel()
    in_buf, in_view = _carve(nb, 16 + el, 0x33)
    in_view.copy_(src)
    out_buf, out_view = _carve(nb, 16 + el, 0x5a)
    mask_buf, mask_view = _carve(n * H * W * 4, 16 + 4, 0xa5)
    depth = world.depth[:n].contiguous()
    p = world.aug.plan(RATE, IDX[:n])
    sims, fog = np.ascontiguousarray(p['sims']), np.ascontiguousarray(p['fog'])
    b = hb.rr_tensor_batch()
    b.n, b.H, b.W, b.dtype = n, H, W, CODE[dtype]
    b.layout = hb.RR_LAYOUT_INTERLEAVED if interleaved else hb.RR_LAYOUT_PLANAR
    b.images, b.depth = in_view.data_ptr(), depth.data_ptr()
    b.sims, b.fog, b.drops_cap = sims.ctypes.data, fog.ctypes.data, p['drops_cap']
    b.rainy_out, b.mask_out = out_view.data_ptr(), mask_view.data_ptr()
    assert b.images % 16 == el and b.rainy_out % 16 == el
    torch.cuda.synchronize()
    world.aug._hip.augment_frames_device(b)                              # on the context's stream: the call waits for the result
    assert torch.equal(out_view, _frames_bytes(want, interleaved))
    assert torch.equal(mask_view, want_mask.contiguous().reshape(-1).view(torch.uint8))
    assert torch.equal(in_buf[16 + el:16 + el + nb], src) and bool((in_buf[:16 + el] == 0x33).all()) and bool((in_buf[16 + el + nb:] == 0x33).all())
    assert bool((out_buf[:16 + el] == 0x5a).all()) and bool((out_buf[16 + el + nb:] == 0x5a).all())
    assert bool((mask_buf[:20] == 0xa5).all()) and bool((mask_buf[20 + n * H * W * 4:] == 0xa5).all())


# ---- 4. a rig ------------------------------------------------------------------------------------------------------------------------------
def test_rig_batches_with_channels_last_views(world, streaks_db):
    aug = augment.RainAugment('fmtcam', streaks_db=streaks_db, particle_model='rig', rig=rigmod.Rig.stereo(0.54))
    try:
        dep = torch.stack([world.depth, world.depth + 1.0], dim=1)
        for dtype in (torch.uint8, torch.bfloat16):
            x = torch.stack([world.x[dtype], world.x[dtype].flip(0)], dim=1)                                 # [3, 2, 3, H, W]
            want, want_mask = aug(x, dep, RATE, IDX)
            x_cl = x.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
            keep = x_cl.clone()
            assert x_cl.shape == x.shape and not x_cl.is_contiguous() and x_cl.stride()[2:] == (1, 3 * W, 3)
            rainy, mask = aug(x_cl, dep, RATE, IDX)
            assert rainy.dtype == dtype and rainy.shape == x.shape and rainy.stride() == x_cl.stride()
            assert torch.equal(rainy, want) and torch.equal(mask, want_mask) and torch.equal(_bits(x_cl), _bits(keep))
            assert all(float(want_mask[i, v].max()) > 0 for i in range(N) for v in range(2))
            one_cl = x[1:2].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)                       # one instant
            one, one_mask = aug(one_cl, dep[1:2], RATE, IDX[1:2])
            assert one.stride() == one_cl.stride() and torch.equal(one, want[1:2]) and torch.equal(one_mask, want_mask[1:2])
    finally:
        aug.close()


# ---- 5. source_size= -----------------------------------------------------------------------------------------------------------------------
def test_every_new_format_through_the_input_resize(built, streaks_db, monkeypatch):
    tgr = importlib.import_module('test_gpu_input_resize')
    tgr._small_camera(monkeypatch, 2)                                    # a 160 x 96 sensor rendered at scale 2: 48 x 80 frames
    SH, SW = tgr.SH, tgr.SW
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', source_size=(SH, SW))
    try:
        assert aug.frame_size() == (SH // 2, SW // 2)
        idx = [0, 1, 2]
        dep = _depth(N, SH // 2, SW // 2, seed=5).to(DEV)
        x8 = _images(torch.uint8, N, SH, SW, seed=5).to(DEV)
        want8, mask8 = aug(x8, dep, 25, idx)
        assert want8.shape == (N, 3, SH // 2, SW // 2) and all(float(mask8[i].max()) > 0 for i in range(N))
        r, m = aug(x8.contiguous(memory_format=CL), dep, 25, idx)
        assert torch.equal(r, want8) and torch.equal(m, mask8) and r.is_contiguous(memory_format=CL) and not r.is_contiguous()
        xf = _images(torch.float32, N, SH, SW, seed=5).to(DEV)
        wantf, maskf = aug(xf, dep, 25, idx)
        r, m = aug(xf.contiguous(memory_format=CL), dep, 25, idx)
        assert torch.equal(r, wantf) and torch.equal(m, maskf) and torch.equal(m, mask8) and r.is_contiguous(memory_format=CL)
        for dtype in HALVES:
            xh = _images(dtype, N, SH, SW, seed=5).to(DEV)
            wanth, maskh = aug(xh.float(), dep, 25, idx)                 # planar float32 on the widened values, narrowed
            for x in (xh, xh.contiguous(memory_format=CL)):
                r, m = aug(x, dep, 25, idx)
                assert r.dtype == dtype and torch.equal(r, wanth.to(dtype)) and torch.equal(m, maskh), (dtype, x.stride())
            assert r.is_contiguous(memory_format=CL)
            one, _ = aug(x[:1], dep[:1], 25, idx[:1])                                                         # one frame (interleaved)
            assert torch.equal(one, wanth[:1].to(dtype))
    finally:
        aug.close()


# ---- 6. lens= ------------------------------------------------------------------------------------------------------------------------------
def test_lens_pass_on_channels_last_bytes(world, streaks_db):
    L = lens.LensDrops(H, W, count=8, radius=(2, 9), seed=8)
    both = augment.RainAugment('fmtcam', streaks_db=streaks_db, lens=L, return_lens_alpha=True)
    la = augment.LensAugment(L, return_alpha=True)
    try:
        assert all(len(L.table(f)) >= 1 for f in IDX)
        x = world.x[torch.uint8]
        x_cl = x.contiguous(memory_format=CL)
        want, want_mask, want_alpha = both(x, world.depth, RATE, IDX)
        rainy, mask, alpha = both(x_cl, world.depth, RATE, IDX)
        assert rainy.stride() == x_cl.stride() and torch.equal(rainy, want) and torch.equal(mask, want_mask) and torch.equal(alpha, want_alpha)
        assert float(alpha.max()) > 0 and alpha.is_contiguous() and not torch.equal(want, world.planar(torch.uint8)[0])
        assert torch.equal(mask, world.planar(torch.uint8)[1])
        # LensAugment: the lens pass alone, on the rainy frames
        r0 = world.planar(torch.uint8)[0]
        w1, a1 = la(r0, IDX)
        g1, ga1 = la(r0.contiguous(memory_format=CL), IDX)
        assert g1.stride() == x_cl.stride() and torch.equal(g1, w1) and torch.equal(ga1, a1) and torch.equal(w1, want)
        g2, _ = la(r0[:1].contiguous(memory_format=CL), IDX[:1])                                              # one frame
        assert torch.equal(g2, w1[:1])
        # the combinations the lens pass does not take: refused before any GPU work
        for bad in (world.x[torch.float16], world.x[torch.bfloat16], world.x[torch.bfloat16].contiguous(memory_format=CL),
                    world.x[torch.float32].contiguous(memory_format=CL)):
            with pytest.raises(ValueError, match='lens= takes uint8 batches'):
                both(bad, world.depth, RATE, IDX)
        with pytest.raises(TypeError, match='uint8 or float32'):
            la(world.x[torch.float16], IDX)
        rf, _, _ = both(world.x[torch.float32], world.depth, RATE, IDX)                                      # planar float32 runs as before
        assert rf.dtype == torch.float32 and rf.is_contiguous()
    finally:
        both.close()
        la.close()


# ---- 7. a side stream ----------------------------------------------------------------------------------------------------------------------
def test_interleaved_bfloat16_on_a_side_stream(world):
    want, want_mask = world.planar(torch.bfloat16)
    src, dsrc = world.x[torch.bfloat16].contiguous(memory_format=CL), world.depth
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        # inputs made by torch kernels on s right before the call, no synchronisation in between
        img = torch.flip(torch.flip(src, [3]), [3])
        dep = dsrc * 1.0
        assert img.stride() == src.stride()
        got = world.aug(img, dep, RATE, IDX)
        one = world.aug(torch.flip(torch.flip(src[2:3], [3]), [3]), dsrc[2:3] * 1.0, RATE, IDX[2:3])          # one frame
    assert torch.equal(got[0], want) and torch.equal(got[1], want_mask) and got[0].stride() == src.stride()
    assert torch.equal(one[0], want[2:3]) and torch.equal(one[1], want_mask[2:3]) and one[0].is_contiguous(memory_format=CL)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_e_arg_and_leave_the_context_usable(world):
    want, want_mask = world.planar(torch.float16)
    x = world.x[torch.float16]
    buf = torch.zeros((x.numel() * 2 + 64,), dtype=torch.uint8, device=DEV)
    buf[16:16 + x.numel() * 2].copy_(x.reshape(-1).view(torch.uint8))
    rainy = torch.empty_like(x)
    mask = torch.empty((N, 1, H, W), dtype=torch.float32, device=DEV)
    p = world.aug.plan(RATE, IDX)
    sims, fog = np.ascontiguousarray(p['sims']), np.ascontiguousarray(p['fog'])

    def call(dtype=hb.RR_TENSOR_F16, layout=0, images_off=16, out=None, n=N):
        b = hb.rr_tensor_batch()
        b.n, b.H, b.W, b.dtype, b.layout = n, H, W, dtype, layout
        b.images, b.depth = buf.data_ptr() + images_off, world.depth.data_ptr()
        b.sims, b.fog, b.drops_cap = sims.ctypes.data, fog.ctypes.data, p['drops_cap']
        b.rainy_out, b.mask_out = rainy.data_ptr() if out is None else out, mask.data_ptr()
        torch.cuda.synchronize()
        world.aug._hip.augment_frames_device(b)

    def good(n=N):
        rainy.zero_()
        mask.zero_()
        call(n=n)                                                        # (the first n frames of the batch: the records are per frame)
        assert torch.equal(rainy[:n], want[:n]) and torch.equal(mask[:n], want_mask[:n])
        assert not bool(rainy[n:].any()) and not bool(mask[n:].any())

    good()
    good(1)                                                              # one frame
    with pytest.raises(RuntimeError, match=r'rr_augment_frames_device failed \(-1\): rr_augment_frames_device'):
        call(n=1, layout=2)
    good(1)
    for kw in (dict(layout=2), dict(layout=-1), dict(dtype=2), dict(dtype=hb.RR_TENSOR_U8_HWC), dict(dtype=hb.RR_TENSOR_U8_HWC, layout=1), dict(dtype=6),
               dict(images_off=17), dict(dtype=hb.RR_TENSOR_BF16, images_off=17), dict(out=rainy.data_ptr() + 1),
               dict(dtype=hb.RR_TENSOR_F32, images_off=18), dict(dtype=hb.RR_TENSOR_F32, layout=1, out=rainy.data_ptr() + 2)):
        with pytest.raises(RuntimeError, match=r'rr_augment_frames_device failed \(-1\): rr_augment_frames_device'):
            call(**kw)
        good()                                                           # nothing was enqueued, the context is what it was
