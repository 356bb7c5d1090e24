"""GPU tier of the drops on the lens (rr_lens_drops_device, k_lens_drops), one process.

  1. device output == the numpy statement (tools/lens.py apply_numpy) on the scenes of tests/lens_cases.py: float32 bit for bit, bytes
     byte for byte, alpha_out bit for bit, every pixel with A == 0 the input; no alpha asked for: the same images;
  2. every RR_E_ARG of include/rainhip.h, nothing written by a refused call, and the next good call correct;
  3. the caller's stream: enqueued on a non-default torch stream behind the kernels that produce `images`, read back on that stream;
  4. RainAugment(lens=L) == LensAugment(L) on the output of the same augmenter without a lens (uint8 and float32, B = 2), the streak
     mask unchanged, return_lens_alpha the statement's alpha;
  5. a stereo rig: each view wears its own table;
  6. two calls give equal bytes."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import helpers as h
import lens_cases as lc
from test_gpu_augment import DEV, _planar, _scene, streaks_db          # noqa: F401  (streaks_db: a fixture)
from test_lens_host import _bad_tables, _pack

pytestmark = pytest.mark.gpu

augment = importlib.import_module('rain-rendering_amd.augment')
rigmod = importlib.import_module('rain-rendering_amd.rig')
lens = lc.lens
RR_E_ARG = -1
KH, KW = 375, 1242                                         # KITTI's frames


@pytest.fixture(scope='module')
def rh(built):
    ctx = h.hb.RainHip(0)
    yield ctx
    ctx.close()


def _run(rh, img, tabs, weights=lc.WEIGHTS, want_alpha=True, stream=None):
    """The lens pass on host images through device tensors: (out, alpha) as numpy.  The outputs start out as garbage."""
    n, _, H, W = img.shape
    d_img = torch.from_numpy(np.array(img)).to(DEV)
    d_out = torch.full_like(d_img, 3)
    d_alpha = torch.full((n, H, W), -1.0, dtype=torch.float32, device=DEV) if want_alpha else None
    torch.cuda.synchronize()
    rh.lens_drops_device(d_img.data_ptr(), d_out.data_ptr(), n, H, W, img.dtype == np.float32, tabs, weights,
                         alpha_ptr=None if d_alpha is None else d_alpha.data_ptr(), stream=stream)
    return d_out.cpu().numpy(), None if d_alpha is None else d_alpha.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. device == statement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", lc.SCENES)
def test_device_equals_the_statement(rh, name, dtype):
    img, tabs, want, want_alpha = lc.scene(name, dtype)
    got, alpha = _run(rh, img, tabs)
    diff = np.argwhere(got != want)
    print('%s %s: %d of %d values differ' % (name, dtype, len(diff), want.size), diff[:5].tolist())
    assert _same_bits(got, want)
    assert _same_bits(alpha, want_alpha)
    keep = np.broadcast_to(alpha[:, None] == 0, got.shape)
    assert _same_bits(got[keep], img[keep]) and keep.any() and not keep.all()
    got2, none = _run(rh, img, tabs, want_alpha=False)                 # no alpha asked for: the same images
    assert none is None and _same_bits(got2, want)


# ---- 2. refusals ---------------------------------------------------------------------------------------------------
def _batch(d_img, d_out, d_alpha, tabs, weights=lc.WEIGHTS, cap=None, counts=None, dtype=None):
    n, _, H, W = d_img.shape
    c, drops, cp = _pack(tabs)
    counts = c if counts is None else np.asarray(counts, np.int32)
    radius, w = np.ascontiguousarray(weights[0], np.int32), np.ascontiguousarray(weights[1], np.float32)
    b = h.hb.rr_lens_batch()
    b.n, b.H, b.W = n, H, W
    b.dtype = (1 if d_img.dtype == torch.float32 else 0) if dtype is None else dtype
    b.images, b.out, b.alpha_out = d_img.data_ptr(), d_out if isinstance(d_out, int) else d_out.data_ptr(), d_alpha
    b.counts, b.drops, b.cap = counts.ctypes.data, drops.ctypes.data, cp if cap is None else cap
    b.n_classes, b.class_radius, b.weights = len(radius), radius.ctypes.data, w.ctypes.data
    return b, (counts, drops, radius, w)


def test_refusals(rh):
    img, tabs, want, want_alpha = lc.scene('odd', 'uint8')
    d_img = torch.from_numpy(np.array(img[:1])).to(DEV)
    d_out = torch.full_like(d_img, 3)
    d_alpha = torch.full((1, lc.H, lc.W), -1.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    lib, hnd = rh.lib, rh.h
    n_bytes = d_img.numel()

    def refused(what, b_keep):
        rc = lib.rr_lens_drops_device(hnd, ctypes.byref(b_keep[0]), None)
        assert rc == RR_E_ARG, (what, rc)
        assert rh.lib.rr_last_error(hnd).decode().startswith('rr_lens_drops_device'), what

    one = [tabs[0]]
    for name, t, _ in _bad_tables():
        refused(name, _batch(d_img, d_out, d_alpha.data_ptr(), [t]))
    refused('out == images', _batch(d_img, d_img, None, one))
    refused('out overlaps images', _batch(d_img, d_img.data_ptr() + n_bytes - 1, None, one))
    refused('images overlaps out', _batch(d_img, d_img.data_ptr() - n_bytes + 1, None, one))
    refused('alpha == out', _batch(d_img, d_out, d_out.data_ptr(), one))
    refused('alpha overlaps images', _batch(d_img, d_out, d_img.data_ptr() + 4, one))
    refused('count above cap', _batch(d_img, d_out, None, one, cap=4))
    refused('count above RR_MAX_LENS_DROPS', _batch(d_img, d_out, None, [np.repeat(tabs[0][:1], 129)]))
    refused('negative count', _batch(d_img, d_out, None, one, counts=[-1]))
    refused('radius 16', _batch(d_img, d_out, None, one, weights=([0, 4, 16], lc.WEIGHTS[1])))
    refused('radius -1', _batch(d_img, d_out, None, one, weights=([0, -1, 15], lc.WEIGHTS[1])))
    refused('17 classes', _batch(d_img, d_out, None, one, weights=([0] * 17, lc.WEIGHTS[1])))
    refused('no class', _batch(d_img, d_out, None, one, weights=([], lc.WEIGHTS[1])))
    w = lc.WEIGHTS[1].copy()
    w[2, 3] = np.inf
    refused('a weight that is not finite', _batch(d_img, d_out, None, one, weights=(lc.WEIGHTS[0], w)))
    refused('dtype', _batch(d_img, d_out, None, one, dtype=2))
    b, keep = _batch(d_img, d_out, None, one)
    b.n = 0
    refused('n = 0', (b, keep))
    b, keep = _batch(d_img, d_out, None, one)
    b.images = None
    refused('null images', (b, keep))
    b, keep = _batch(d_img, d_out, None, one)
    b.drops = None
    refused('null drops', (b, keep))
    assert lib.rr_lens_drops_device(hnd, None, None) == RR_E_ARG
    torch.cuda.synchronize()
    assert bool((d_out == 3).all()) and bool((d_alpha == -1).all())    # a refused call enqueues nothing
    # the next good call is correct
    got, alpha = _run(rh, img, tabs)
    assert _same_bits(got, want) and _same_bits(alpha, want_alpha)


# ---- 3. the caller's stream ----------------------------------------------------------------------------------------
def test_on_the_callers_stream_behind_the_producer(rh):
    img, tabs, want, want_alpha = lc.scene('odd', 'float32')
    n = len(tabs)
    half = torch.from_numpy(np.array(img) * np.float32(0.5)).to(DEV)
    busy = torch.ones(1 << 25, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    assert s.cuda_stream != 0
    with torch.cuda.stream(s):
        for _ in range(8):                                             # work in front of the producer, so that it has not run when the call is made
            busy = busy * 1.0001 + 0.5
        d_img = half + half                                            # the kernel that produces `images`: x / 2 + x / 2 == x
        d_out = torch.empty_like(d_img)
        d_alpha = torch.empty((n, lc.H, lc.W), dtype=torch.float32, device=DEV)
        rh.lens_drops_device(d_img.data_ptr(), d_out.data_ptr(), n, lc.H, lc.W, True, tabs, lc.WEIGHTS, alpha_ptr=d_alpha.data_ptr(),
                             stream=s.cuda_stream)
        flipped = d_out.flip(0)                                        # a consumer on the same stream
        got, alpha = flipped.cpu().numpy()[::-1], d_alpha.cpu().numpy()          # (these copies wait for stream s alone)
    assert _same_bits(np.ascontiguousarray(got), want) and _same_bits(alpha, want_alpha)


# ---- 4. RainAugment(lens=) -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def kitti(built, streaks_db):
    L = lens.LensDrops(KH, KW, count=24, seed=3)
    kw = dict(streaks_db=streaks_db, sequence='data_object/training')
    plain = augment.RainAugment('kitti', **kw)
    both = augment.RainAugment('kitti', lens=L, return_lens_alpha=True, **kw)
    two = augment.RainAugment('kitti', lens=L, **kw)
    alone = augment.LensAugment(L, return_alpha=True)
    yield L, plain, both, two, alone
    for a in (plain, both, two, alone):
        a.close()


@pytest.mark.parametrize("dtype", ['uint8', 'float32'])
def test_rain_augment_with_a_lens(kitti, dtype):
    L, plain, both, two, alone = kitti
    bgr, depth = _scene(2, KH, KW, seed=60)
    if dtype == 'float32':
        bgr = (bgr.astype(np.float64) / 255.0).astype(np.float32)
    images, d = _planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV)
    idx = [4, 31]
    assert len(L.table(4)) > 5 and L.table(4).tobytes() != L.table(31).tobytes()
    rainy0, mask0 = plain(images, d, 25, idx)
    rainy, mask, alpha = both(images, d, 25, idx)
    assert rainy.dtype == images.dtype and tuple(alpha.shape) == (2, 1, KH, KW) and alpha.dtype == torch.float32
    want, want_alpha = alone(rainy0, idx)
    assert torch.equal(rainy, want) and torch.equal(alpha, want_alpha)
    assert torch.equal(mask, mask0) and float(mask.max()) > 0          # the streak mask is the one without a lens
    assert not torch.equal(rainy, rainy0)
    # ... and both are the statement's
    st, st_alpha = lens.apply_numpy(rainy0.cpu().numpy(), [L.table(f) for f in idx], L.weights(), alpha=True)
    assert _same_bits(rainy.cpu().numpy(), st) and _same_bits(alpha.cpu().numpy()[:, 0], st_alpha)
    assert ((st_alpha > 0) & (st_alpha < 1)).any() and (st_alpha == 1).any()
    # two return values without return_lens_alpha; determinism: two calls give equal bytes
    r2 = two(images, d, 25, idx)
    assert len(r2) == 2 and torch.equal(r2[0], rainy) and torch.equal(r2[1], mask)
    again = both(images, d, 25, idx)
    assert all(torch.equal(a, b) for a, b in zip(again, (rainy, mask, alpha)))


def test_lens_augment_alone(built):
    L = lens.LensDrops(lc.H, lc.W, count=6, radius=(2, 9), seed=8)
    img = lc.images(3, lc.H, lc.W, np.uint8)
    idx = [0, 9, 400]
    la = augment.LensAugment(L)
    try:
        out = la(torch.from_numpy(img).to(DEV), idx)
        assert isinstance(out, torch.Tensor) and _same_bits(out.cpu().numpy(), lens.apply_numpy(img, [L.table(f) for f in idx], L.weights()))
        assert torch.equal(out, la(torch.from_numpy(img).to(DEV), np.array(idx)))
    finally:
        la.close()


# ---- 5. a rig ------------------------------------------------------------------------------------------------------
def test_each_view_of_a_rig_wears_its_own_table(built, streaks_db):
    L = lens.LensDrops(KH, KW, count=24, seed=5)
    kw = dict(streaks_db=streaks_db, sequence='data_object/training', particle_model='rig', rig=rigmod.Rig.stereo(0.54))
    plain, both = augment.RainAugment('kitti', **kw), augment.RainAugment('kitti', lens=L, return_lens_alpha=True, **kw)
    views = [augment.LensAugment(L.for_view(v), return_alpha=True) for v in (0, 1)]
    try:
        bgr, depth = _scene(1, KH, KW, seed=70)
        img, d = _planar(bgr).to(DEV), torch.from_numpy(depth).to(DEV)
        images, dep = torch.stack([img, img], dim=1), torch.stack([d, d], dim=1)
        idx = [12]
        rainy0, mask0 = plain(images, dep, 25, idx)
        rainy, mask, alpha = both(images, dep, 25, idx)
        assert tuple(rainy.shape) == (1, 2, 3, KH, KW) and tuple(alpha.shape) == (1, 2, 1, KH, KW) and torch.equal(mask, mask0)
        for v in (0, 1):
            want, want_alpha = views[v](rainy0[:, v].contiguous(), idx)
            assert torch.equal(rainy[:, v], want) and torch.equal(alpha[:, v], want_alpha), v
        assert not torch.equal(alpha[:, 0], alpha[:, 1]) and float(alpha[:, 0].max()) == 1.0 == float(alpha[:, 1].max())
    finally:
        for a in [plain, both] + views:
            a.close()


# ---- 6. determinism ------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes(rh):
    img, tabs, want, _ = lc.scene('odd', 'uint8')
    a, aa = _run(rh, img, tabs)
    b, ab = _run(rh, img, tabs)
    assert _same_bits(a, b) and _same_bits(aa, ab) and _same_bits(a, want)
