"""GPU tier: the compositors' epilogue -- output pointers read once from the frame's descriptor, every store in one burst --
on the frames of tests/compositor_outputs.py: one call of three 24 x 40 frames that differ in the optional outputs they ask
for (mask_f64 only, mask_i32 only, both) and in their drop tables, with lanes whose second pixel is dead, waves that own no
pixel, drops across both tile seams and one input pixel outside [0, 1] that no drop reaches (code 65535 of the 16-bit
composite).  Through rr_render_frames_device, the entry that hands the caller's pointers -- and nulls -- to the kernels as
they are.  Every output buffer is poisoned first and compared WHOLE with the host emulation: the mask bit for bit, the image
within 1 LSB (the bars of tests/compositor_cases.py check)."""
import numpy as np
import pytest
import torch

import compositor_cases as cc
import compositor_outputs as co
import helpers as h

pytestmark = pytest.mark.gpu

# name -> (rr_set_option settings, the kernels that run)
CONFIGS = {
    'codes16': ({}, 'k_composite32, 16-bit codes, k_finalize16'),
    'floats': (dict(RR_OPT_WILD_PIXELS=1), 'k_composite32, three floats, k_finalize'),
    'composite_f64': (dict(RR_OPT_COMPOSITE_F64=1), 'k_composite, k_finalize'),
}
POISON_F64, POISON_I32, POISON_U8, GUARD = -777.25, -777, 0xA5, 64


@pytest.fixture(scope='module')
def frames(built, tmp_path_factory):
    """(case, tables, backgrounds, host-emulation references); the census is a condition of every test below."""
    tpl = cc.Templates(tmp_path_factory.mktemp('tpl'))
    c, tables, bgs = co.build(tmp_path_factory.mktemp('outputs'), tpl)
    refs = co.references(c, tables, bgs)
    n = co.census(c, tables, bgs, refs)
    assert n['first_only'] > 0 and n['both_dead'] > 0 and n['null_outputs'] == 2 and n['code_65535_pixels'] == 1 and n['seam_drops'] >= 2
    return c, tables, bgs, refs


def _run(c, tables, bgs, opts):
    """One rr_render_frames_device call on torch tensors; per frame dict(image_u8, mask | None, mask_i32 | None, status)."""
    dev = torch.device('cuda', 0)
    nf = len(tables)
    dbl = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    t_env, t_om = dbl(c.env), dbl(c.scene.omega)
    fin, fout = (h.hb.rr_frame_in * nf)(), (h.hb.rr_frame_out * nf)()
    keep, bufs = [t_env, t_om], []
    for k, (idx, bg, (want_f64, want_i32)) in enumerate(zip(tables, bgs, co.WANTS)):
        drops = np.ascontiguousarray(c.drops[idx])
        t_bg = dbl(bg)
        t_drops = torch.from_numpy(drops.view(np.uint8).reshape(-1).copy()).to(dev)
        t_rgb = torch.full((GUARD + co.H * co.W * 3 + GUARD,), POISON_U8, dtype=torch.uint8, device=dev)
        t_mask = torch.full((co.H * co.W + 2 * GUARD,), POISON_F64, dtype=torch.float64, device=dev) if want_f64 else None
        t_mi = torch.full((co.H * co.W + 2 * GUARD,), POISON_I32, dtype=torch.int32, device=dev) if want_i32 else None
        t_status = torch.full((len(drops),), POISON_I32, dtype=torch.int32, device=dev)
        keep += [t_bg, t_drops]
        bufs.append((t_rgb, t_mask, t_mi, t_status))
        fi, fo = fin[k], fout[k]
        fi.H, fi.W, fi.He, fi.We = co.H, co.W, c.env.shape[0], c.env.shape[1]
        fi.bg = fi.rainy_bg = t_bg.data_ptr()
        fi.env_xyY, fi.omega = t_env.data_ptr(), t_om.data_ptr()
        fi.drops, fi.n_drops, fi.strategy, fi.opacity_attenuation = t_drops.data_ptr(), len(drops), 0, 1.0
        fo.rainy_rgb = t_rgb.data_ptr() + GUARD
        fo.mask_f64 = t_mask.data_ptr() + 8 * GUARD if want_f64 else None
        fo.mask_i32 = t_mi.data_ptr() + 4 * GUARD if want_i32 else None
        fo.drop_status = t_status.data_ptr()
    torch.cuda.synchronize()
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(c.scene.db.streaks_light)
        rh.set_camera(c.scene.cam)
        for o, v in opts.items():
            rh.set_option(getattr(h.hb, o), v)
        rh.render_frames_device(fin, fout, nf)
        assert rh.synchronize()
        outs = []
        for k, (t_rgb, t_mask, t_mi, t_status) in enumerate(bufs):
            o = dict(status=t_status.cpu().numpy(), mask=None, mask_i32=None)
            for key, t, size, poison in (('image_u8', t_rgb, co.H * co.W * 3, POISON_U8), ('mask', t_mask, co.H * co.W, POISON_F64),
                                         ('mask_i32', t_mi, co.H * co.W, POISON_I32)):
                if t is None:
                    continue
                a = t.cpu().numpy()
                assert (a[:GUARD] == poison).all() and (a[GUARD + size:] == poison).all(), ('frame %d' % k, key, 'written outside the array')
                o[key] = a[GUARD:GUARD + size].reshape((co.H, co.W, 3) if key == 'image_u8' else (co.H, co.W)).copy()
            outs.append(o)
        return outs
    finally:
        rh.close()


@pytest.mark.parametrize('config', list(CONFIGS))
def test_every_output_of_every_frame(frames, config):
    c, tables, bgs, refs = frames
    outs = _run(c, tables, bgs, CONFIGS[config][0])
    geom = cc.GEOM64 if config == 'composite_f64' else cc.GEOM32
    for k, (out, ref, (want_f64, want_i32)) in enumerate(zip(outs, refs, co.WANTS)):
        tag = 'frame %d (%s)' % (k, CONFIGS[config][1])
        assert np.array_equal(out['status'], ref['status']), (tag, out['status'], ref['status'])
        assert (out['mask'] is not None) == want_f64 and (out['mask_i32'] is not None) == want_i32
        found = {}
        if want_f64:
            diff = out['mask'] != ref['mask']                 # whole array: a pixel no drop reaches is 0.0, not the poison
            if diff.any():
                found['mask'] = cc.where(c, diff, geom)
        if want_i32:
            diff = out['mask_i32'] != ref['mask_i32']
            if diff.any():
                found['mask_i32'] = cc.where(c, diff, geom)
        diff = (np.abs(out['image_u8'].astype(int) - ref['image_u8'].astype(int)) > 1).any(axis=2)
        if diff.any():
            found['image_u8'] = cc.where(c, diff, geom)
        assert not found, '%s differs from the host emulation: %s' % (tag, found)
    assert outs[0]['mask'].max() > 0 and outs[1]['mask_i32'].max() > 0
    # the tables of frames 0 and 1 differ: a pointer taken from the neighbour's descriptor would have shown above
    assert not np.array_equal(outs[0]['mask'], refs[1]['mask'])
