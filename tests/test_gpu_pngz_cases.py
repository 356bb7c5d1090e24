"""GPU tier of the PNG coder's catalogue (tests/pngz_cases.py): k_pngz_blocks / k_pngz_pack through the C ABI, every byte exact.

Every file is held three ways: (a) numpy's Sub filter of the returned image (for the mask file: of the host writer's colour-mapped
mask) is the plain mode's scanlines, (b) zlib inflates the device's stream to those scanlines (and checks its Adler-32), (c) the whole
buffer -- header, length, stream, trailer, or the untouched scanlines of a file that does not fit -- is what the host build of the
same phases (emu_pngz) makes of them.  For the drop-less frames of the catalogue the plain scanlines ARE the case's intended bytes, so
a case cannot miss its target unnoticed.  tests/test_pngz_cases_host.py holds the emulation to zlib on the same inputs and shows on its
trace where each case lands."""
import zlib

import numpy as np
import pytest
import torch

import helpers as h
import lens_cases as lc
import pngz_cases as pc

pytestmark = pytest.mark.gpu
hb = h.hb
SENTINEL = 0xA5


class Ctx:
    def __init__(self, tmp):
        self.sc = h.Scene(tmp, 64, 128, 150, n_frames=2, seed0=31)
        self.env = self.sc.frame_inputs(0)[1]
        self.lut = pc.random_lut()
        self.rh = hb.RainHip(0)
        self.rh.set_streak_db(self.sc.db.streaks_light)
        self.rh.set_camera(self.sc.cam)
        self.rh.set_colormap(self.lut)
        self.rh.profile(True)
        self.none = np.zeros(0, hb.DROP_DTYPE)

    def frame(self, img, drops=None):
        bg = pc.rainy_bg_of(img)
        return dict(bg=bg, rainy_bg=bg, env_xyY=self.env, omega=self.sc.omega, drops=self.none if drops is None else drops)

    def run(self, frames, wants, deflate, slot=0):
        """One batch on `slot`; wants: per frame the files asked for, a subset of ('rainy_png', 'mask_png').  Returns (outs, launches of
        the coder's scope)."""
        H, W = frames[0]['bg'].shape[:2]
        n = H * (1 + 4 * W)
        outs, spare = [], []
        for fr, want in zip(frames, wants):
            o = dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W)), status=np.zeros(len(fr['drops']), np.int32))
            block = np.full((3, n), SENTINEL, np.uint8)            # [rainy_png | mask_png | a guard], back to back
            for k, key in enumerate(BOTH):
                if key in want:
                    o[key] = block[k]
            outs.append(o)
            spare.append((block, [k for k, key in enumerate(BOTH) if key not in want] + [2]))
        self.rh.set_option(hb.RR_OPT_PNG_DEFLATE, 1 if deflate else 0)
        try:
            self.rh.profile_reset()
            self.rh.pipeline_submit(slot, frames, outs)
            if not self.rh.pipeline_wait(slot):                     # (the tile arena grew: once more)
                self.rh.profile_reset()
                self.rh.pipeline_submit(slot, frames, outs)
                assert self.rh.pipeline_wait(slot)
            launches = self.rh.profile_read().get('k_pngz', (0, 0.0))[0]
        finally:
            self.rh.set_option(hb.RR_OPT_PNG_DEFLATE, 0)
        for f, (block, untouched) in enumerate(spare):          # a file that was not asked for (and the bytes behind the files) stay
            for k in untouched:
                assert (block[k] == SENTINEL).all(), ('frame %d' % f, (BOTH + ('guard',))[k], 'was not asked for and was written')
        return outs, launches


@pytest.fixture(scope="module")
def ctx(built, tmp_path_factory):
    c = Ctx(tmp_path_factory.mktemp('pngz'))
    yield c
    c.rh.close()


def check_coded(tag, plain, coded):
    """References (b) and (c) of one file: `plain` the plain mode's scanlines, `coded` the buffer of the run with RR_OPT_PNG_DEFLATE."""
    n = plain.size
    total, want = pc.emu_pngz(plain)
    if coded[:4].tobytes() == pc.MAGIC:
        L = int(coded[4:8].view(np.uint32)[0])
        assert 0 < L and pc.HEADER + L <= n, (tag, L, n)
        assert zlib.decompress(coded[16:16 + L].tobytes()) == plain.tobytes(), tag                     # (b)
    else:
        assert coded[0] <= 4 and np.array_equal(coded, plain), (tag, 'neither a stream nor the scanlines')
    if not np.array_equal(coded, want):                                                                   # (c)
        bad = np.flatnonzero(coded != want)
        raise AssertionError("%s: %d bytes differ from the emulation's buffer (stream of %d), first at %d" % (tag, bad.size, total, bad[0]))
    return total


def check_plain(tag, out, lut, intended=None):
    """Reference (a) of a frame's files, and the catalogue's aim."""
    if 'rainy_png' in out:
        assert np.array_equal(out['rainy_png'], pc.scanlines_rgb(out['image_u8'])), (tag, 'rainy_png')
        if intended is not None:
            assert np.array_equal(out['rainy_png'], intended), (tag, 'rainy_png', "not the case's intended bytes")
    if 'mask_png' in out:
        assert np.array_equal(out['mask_png'], pc.scanlines_rgba(pc.mask_rgba(out['mask'], lut))), (tag, 'mask_png')


BOTH = ('rainy_png', 'mask_png')


@pytest.mark.parametrize("H,W", list(pc.sizes()), ids=lambda v: str(v))
def test_catalogue_one_batch_per_size(ctx, H, W):
    """Every case of a size in one call, plain and coded.  The mask file of these drop-less frames is the zero-drop mask (hi == lo:
    index 0 of the colour map everywhere)."""
    cases = pc.sizes()[(H, W)]
    frames = [ctx.frame(pc.built(c)[1]) for c in cases]
    plain, launches = ctx.run(frames, [BOTH] * len(cases), False)
    assert launches == 0
    coded, launches = ctx.run(frames, [BOTH] * len(cases), True)
    assert launches >= 1, "RR_OPT_PNG_DEFLATE is on and k_pngz did not run"
    for k, c in enumerate(cases):
        F, img, rows = pc.built(c)
        tag = (c.name, 'frame %d' % k)
        assert np.array_equal(plain[k]['image_u8'], img) and not plain[k]['mask'].any(), tag
        assert np.array_equal(coded[k]['image_u8'], img), tag
        check_plain(tag, plain[k], ctx.lut, intended=rows)
        total = check_coded(tag + ('rainy_png',), plain[k]['rainy_png'], coded[k]['rainy_png'])
        if c.name.startswith('ladder'):                          # kept files are kept, their neighbours coded
            k_kept, k_coded, kept = pc.threshold_pair()
            is_kept = kept[pc.LADDER.index((c.H, c.W))]
            assert (total == 0) == is_kept, tag
            assert (coded[k]['rainy_png'][0] == 1) if is_kept else (coded[k]['rainy_png'][:4].tobytes() == pc.MAGIC), tag
        check_coded(tag + ('mask_png',), plain[k]['mask_png'], coded[k]['mask_png'])


def test_batch_of_four_frames_and_file_kinds(ctx):
    """Four frames of different content in one call: one asks for both files, one for the mask file only, one for the image file only,
    one for neither.  Every file asked for equals the frame run alone; k_pngz_blocks skips the files not asked for."""
    H, W = 47, 43
    Fs = [pc.content(kind, H, W, seed) for kind, seed in (('sparse', 11), ('flat', 0), ('random', 12), ('nozero', 13))]
    imgs = [pc.image_of(F) for F in Fs]
    frames = [ctx.frame(i) for i in imgs]
    wants = [BOTH, ('mask_png',), ('rainy_png',), ()]
    alone = {d: [ctx.run(frames[k:k + 1], [BOTH], d)[0][0] for k in range(4)] for d in (False, True)}
    for deflate in (False, True):
        outs, launches = ctx.run(frames, wants, deflate)
        assert (launches >= 1) == deflate
        for k in range(4):
            assert np.array_equal(outs[k]['image_u8'], imgs[k]), (deflate, k)
            assert set(outs[k]) & set(BOTH) == set(wants[k])
            for key in wants[k]:                                 # (run() pre-fills every buffer with the sentinel: each was written)
                assert outs[k][key][0] in ((1, ord('R')) if deflate else (1,)), (deflate, k, key)
            for key in wants[k]:
                tag = ('four frames', 'deflate %d' % deflate, 'frame %d' % k, key)
                assert np.array_equal(outs[k][key], alone[deflate][k][key]), tag + ('differs from the frame run alone',)
                if deflate:
                    check_coded(tag, alone[False][k][key], outs[k][key])
            if not deflate:
                check_plain(('four frames', 'frame %d' % k), outs[k], ctx.lut, intended=pc.intended(Fs[k]))


def test_mask_file_with_drops_and_a_varied_colour_map(ctx):
    """Drops present and a colour map of 256 distinct RGBA entries: the mask file's scanlines are far from constant; the image file
    carries the rendered streaks."""
    H, W = ctx.sc.H, ctx.sc.W
    img = pc.built(pc.by_name('edge-64x128-sparse'))[1]
    frames = [ctx.frame(img, ctx.sc.product_drops(i)) for i in range(2)]
    plain, _ = ctx.run(frames, [BOTH, BOTH], False)
    coded, launches = ctx.run(frames, [BOTH, BOTH], True)
    assert launches >= 1
    for k in range(2):
        tag = ('drops', 'frame %d' % k)
        assert plain[k]['mask'].max() > 0 and np.array_equal(plain[k]['mask'], coded[k]['mask'])
        assert np.array_equal(plain[k]['image_u8'], coded[k]['image_u8'])
        assert len(np.unique(pc.mask_rgba(plain[k]['mask'], ctx.lut).reshape(-1, 4), axis=0)) > 16, tag
        check_plain(tag, plain[k], ctx.lut)
        for key in BOTH:
            assert check_coded(tag + (key,), plain[k][key], coded[k][key]) > 0


def test_lens_armed_slot_codes_three_files_per_frame(ctx):
    """A slot armed with rr_pipeline_set_lens and alpha_png: k_pngz_blocks<3>, file = 3 * frame + kind.  One frame has no alpha_png
    entry, one asks for the mask file only, one for the image file only."""
    H, W = 64, 128
    n = H * (1 + 4 * W)
    L = lc.lens.LensDrops(H, W, count=12, radius=(2, 12), life_s=(0.2, 0.4), seed=0)
    tables = [L.table(i) for i in range(3)]
    assert all(len(t) >= 4 for t in tables)
    imgs = [pc.built(pc.by_name(name))[1] for name in ('edge-64x128-sparse', 'random-block', 'nozero')]
    frames = [ctx.frame(i) for i in imgs]
    wants = [BOTH, ('mask_png',), ('rainy_png',)]

    def armed(fr, tabs, want, with_alpha, deflate):
        alpha = [np.full(n, SENTINEL, np.uint8) if w else None for w in with_alpha]
        ctx.rh.pipeline_set_lens(1, tabs, L.weights(), H, W, alpha_png=alpha)
        try:
            outs, launches = ctx.run(fr, want, deflate, slot=1)
        finally:
            ctx.rh.pipeline_set_lens(1, None)
        return outs, alpha, launches

    with_alpha = [True, False, True]
    plain, plain_a, launches = armed(frames, tables, [BOTH] * 3, [True] * 3, False)
    assert launches == 0
    coded, coded_a, launches = armed(frames, tables, wants, with_alpha, True)
    assert launches >= 1
    for k in range(3):
        tag = ('lens', 'frame %d' % k)
        assert not np.array_equal(plain[k]['image_u8'], imgs[k]), tag          # the drops on the lens changed the image
        assert np.array_equal(coded[k]['image_u8'], plain[k]['image_u8']), tag
        check_plain(tag, plain[k], ctx.lut)
        label = plain_a[k].reshape(H, 1 + 4 * W)
        px = label[:, 1:].reshape(H, W, 4)
        assert (label[:, 0] == 1).all() and np.array_equal(px[..., 0], px[..., 1]) and np.array_equal(px[..., 0], px[..., 2]), tag
        assert (px[:, 0, 3] == 255).all() and not px[:, 1:, 3].any() and px[..., 0].any(), tag
        for key in wants[k]:
            check_coded(tag + (key,), plain[k][key], coded[k][key])
        if with_alpha[k]:
            assert check_coded(tag + ('alpha_png',), plain_a[k], coded_a[k]) > 0
        alone, alone_a, _ = armed(frames[k:k + 1], tables[k:k + 1], [BOTH], [True], True)
        for key in wants[k]:
            assert np.array_equal(coded[k][key], alone[0][key]), tag + (key, 'differs from the frame run alone')
        if with_alpha[k]:
            assert np.array_equal(coded_a[k], alone_a[0]), tag + ('alpha_png', 'differs from the frame run alone')


# ---- the device-pointer entry: only there can the caller's buffers be misaligned ---------------------------------------------------
GUARD = 64


def _device_run(ctx, imgs, off_png, off_rgb, deflate):
    """rr_render_frames_device on torch tensors: rainy_png and mask_png off_png bytes, rainy_rgb off_rgb bytes behind a 16-byte
    boundary, each inside a sentinel-filled tensor.  Returns per frame dict(image_u8, mask, rainy_png, mask_png) and the launches."""
    dev = torch.device('cuda', 0)
    H, W = imgs[0].shape[:2]
    n, nf = H * (1 + 4 * W), len(imgs)
    t_env = torch.from_numpy(np.ascontiguousarray(ctx.env, np.float64)).to(dev)
    t_om = torch.from_numpy(np.ascontiguousarray(ctx.sc.omega, np.float64)).to(dev)
    fin, fout = (hb.rr_frame_in * nf)(), (hb.rr_frame_out * nf)()
    keep, bufs = [t_env, t_om], []
    for k, img in enumerate(imgs):
        t_bg = torch.from_numpy(pc.rainy_bg_of(img)).to(dev)
        t_mask = torch.zeros((H, W), dtype=torch.float64, device=dev)
        t_rgb = torch.full((GUARD + H * W * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        t_pi = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        t_pm = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        for t in (t_bg, t_mask, t_rgb, t_pi, t_pm):
            assert t.data_ptr() % 16 == 0
        keep += [t_bg, t_mask]
        bufs.append((t_rgb, t_pi, t_pm, t_mask))
        fi, fo = fin[k], fout[k]
        fi.H, fi.W, fi.He, fi.We = H, W, ctx.env.shape[0], ctx.env.shape[1]
        fi.bg = fi.rainy_bg = t_bg.data_ptr()
        fi.env_xyY, fi.omega = t_env.data_ptr(), t_om.data_ptr()
        fi.drops, fi.n_drops, fi.strategy, fi.opacity_attenuation = None, 0, 0, 1.0
        fo.rainy_rgb = t_rgb.data_ptr() + 16 + off_rgb
        fo.mask_f64 = t_mask.data_ptr()
        fo.rainy_png = t_pi.data_ptr() + 16 + off_png
        fo.mask_png = t_pm.data_ptr() + 16 + off_png
    torch.cuda.synchronize()
    ctx.rh.set_option(hb.RR_OPT_PNG_DEFLATE, 1 if deflate else 0)
    try:
        ctx.rh.profile_reset()
        ctx.rh.render_frames_device(fin, fout, nf)
        assert ctx.rh.synchronize()
        launches = ctx.rh.profile_read().get('k_pngz', (0, 0.0))[0]
    finally:
        ctx.rh.set_option(hb.RR_OPT_PNG_DEFLATE, 0)
    outs = []
    for k, (t_rgb, t_pi, t_pm, t_mask) in enumerate(bufs):
        o = dict(mask=t_mask.cpu().numpy())
        for key, t, off, size in (('image_u8', t_rgb, 16 + off_rgb, H * W * 3), ('rainy_png', t_pi, 16 + off_png, n), ('mask_png', t_pm, 16 + off_png, n)):
            a = t.cpu().numpy()
            assert (a[:off] == SENTINEL).all() and (a[off + size:] == SENTINEL).all(), ('frame %d' % k, key, 'bytes around the buffer were written')
            o[key] = a[off:off + size].copy()
        o['image_u8'] = o['image_u8'].reshape(H, W, 3)
        outs.append(o)
    return outs, launches


def test_device_pointer_entry_with_misaligned_buffers(ctx):
    """rr_render_frames_device: the files 1, 7 and 15 bytes, the image 1, 2 and 3 bytes off their boundaries (H * W no multiple of
    four) -- k_pngz_blocks' byte-wise staging loop and k_finalize16's scalar stores -- against a 16-aligned control and all the
    references."""
    H, W = 47, 43
    assert (H * W) % 4 != 0
    cases = [pc.by_name('edge-47x43-sparse'), pc.by_name('edge-47x43-flat')]
    imgs = [pc.built(c)[1] for c in cases]
    control = {}
    for deflate in (False, True):
        control[deflate], launches = _device_run(ctx, imgs, 0, 0, deflate)
        assert (launches >= 1) == deflate
    for off_png, off_rgb in ((0, 0), (1, 1), (7, 2), (15, 3)):
        plain, _ = _device_run(ctx, imgs, off_png, off_rgb, False)
        coded, launches = _device_run(ctx, imgs, off_png, off_rgb, True)
        assert launches >= 1
        for k, c in enumerate(cases):
            tag = (c.name, 'frame %d' % k, 'files +%d, image +%d' % (off_png, off_rgb))
            assert np.array_equal(plain[k]['image_u8'], imgs[k]) and np.array_equal(coded[k]['image_u8'], imgs[k]), tag
            assert not plain[k]['mask'].any(), tag
            check_plain(tag, plain[k], ctx.lut, intended=pc.built(c)[2])
            for key in BOTH:
                assert check_coded(tag + (key,), plain[k][key], coded[k][key]) > 0
                assert np.array_equal(plain[k][key], control[False][k][key]), tag + (key, 'plain differs from the aligned run')
                assert np.array_equal(coded[k][key], control[True][k][key]), tag + (key, 'coded differs from the aligned run')
