"""GPU tier of the input files with chosen filter types (tests/pngrows_cases.py): k_png_unfilter<3> / <2> against the ORIGINAL image
and depth samples.  The pre-pass is fed the filtered scanlines (RR_IN_BG_PNG_ROWS / RR_DEPTH_PNG_ROWS) and its fog layer must equal,
bit for bit, that of the same call fed the original uint8 image and uint16 samples -- a comparison that sees a single sample off by
one (tests/test_pngrows_cases_host.py shows it on the host build of the same arithmetic).  One batch per size: every file of the size,
each with its own filter plans on image and depth map, so the per-file strides are in play as well."""
import importlib

import numpy as np
import pytest

import helpers as h
import pngrows_cases as rc
from oracle import prepass as op

pytestmark = pytest.mark.gpu

fogmod = importlib.import_module('rain-rendering_amd.common.add_attenuation')
RAIN = 25


@pytest.fixture(scope="module")
def ctx(built):
    rh = h.hb.RainHip(0)
    rh.set_prepass_kernels(op.gaussian_kernel(25, 25), op.gaussian_kernel(15, 0))
    consts = fogmod.FogRain(rain_intensity=RAIN, focal=0.006, f_number=6.0, angle=90, exposure=2, camera_gain=20).constants()
    yield rh, consts
    rh.close()


@pytest.mark.parametrize("H,W", rc.SIZES)
def test_chosen_filter_types_give_the_original_samples(ctx, H, W):
    rh, consts = ctx
    files = rc.batch(H, W)
    rh.profile(True)
    rh.profile_reset()
    got = rh.prepass_frames([dict(bg_png_rows=f['image_rows'], shape=(H, W), depth_png_rows=f['depth_rows'], fog=consts) for f in files],
                            want_env=False)
    launches = rh.profile_read().get('k_png_unfilter', (0, 0.0))[0]
    rh.profile(False)
    assert launches >= 1, launches                          # the scanlines went through the kernel
    want = rh.prepass_frames([dict(bg_u8=f['bgr'], depth=f['d16'], fog=consts) for f in files], want_env=False)
    for i, (a, b, f) in enumerate(zip(got, want, files)):
        same = np.array_equal(a['rainy_bg'], b['rainy_bg'])
        where = None if same else np.argwhere((a['rainy_bg'] != b['rainy_bg']).any(axis=-1))[:4].tolist()
        assert same, "%dx%d file %d (image plan %s..., depth plan %s...): fog layer differs first at %s" % (
            H, W, i, f['image_plan'][:3].tolist(), f['depth_plan'][:3].tolist(), where)
        assert b['rainy_bg'].std() > 0


def test_batch_of_three_files_with_different_plans(ctx):
    """Three files in one call equal each file alone: the per-file rows_stride / out_stride."""
    rh, consts = ctx
    H, W = 129, 65
    files = [rc.batch(H, W)[k] for k in (1, 17, 31)]
    assert len({tuple(f['image_plan'].tolist()) for f in files}) == 3
    fr = [dict(bg_png_rows=f['image_rows'], shape=(H, W), depth_png_rows=f['depth_rows'], fog=consts) for f in files]
    together = rh.prepass_frames(fr, want_env=False)
    for i in range(3):
        alone = rh.prepass_frames(fr[i:i + 1], want_env=False)[0]
        orig = rh.prepass_frames([dict(bg_u8=files[i]['bgr'], depth=files[i]['d16'], fog=consts)], want_env=False)[0]
        assert np.array_equal(together[i]['rainy_bg'], alone['rainy_bg']), i
        assert np.array_equal(alone['rainy_bg'], orig['rainy_bg']), i
