"""CPU tier of the drops on the lens: the g++ build of csrc/rr_lens.h against its numpy statement (tools/lens.py
apply_numpy), bit for bit; the generator LensDrops; argument checks; the ABI."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import helpers as h
import lens_cases as lc

lens = lc.lens
RR_E_ARG = -1


@pytest.fixture(scope='module')
def emu(built):
    lib = ctypes.CDLL(os.path.join(h.ROOT, 'tests', 'hostemu', 'liblensemu.so'))
    lib.rr_emu_lens_apply.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 2 + [ctypes.c_void_p] * 2
    lib.rr_emu_lens_check.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 2 + [ctypes.c_void_p] * 2 + \
                                     [ctypes.c_char_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]
    return lib


def _pack(tables):
    counts = np.array([len(t) for t in tables], np.int32)
    cap = max(1, int(counts.max()))
    drops = np.zeros((len(tables), cap), lens.LENS_DROP_DTYPE)
    for f, t in enumerate(tables):
        drops[f, :len(t)] = t
    return counts, drops, cap


def _emu_apply(emu, img, tables, weights):
    n, _, H, W = img.shape
    counts, drops, cap = _pack(tables)
    radius, w = lens.check_weights(weights)
    out = np.full_like(img, 7)
    alpha = np.full((n, H, W), -1.0, np.float32)
    rc = emu.rr_emu_lens_apply(n, H, W, 1 if img.dtype == np.float32 else 0, img.ctypes.data, out.ctypes.data, alpha.ctypes.data,
                               counts.ctypes.data, drops.ctypes.data, cap, len(radius), radius.ctypes.data, w.ctypes.data)
    assert rc == 0
    return out, alpha


def _emu_check(emu, tables, H, W, weights=lc.WEIGHTS, cap=None, counts=None):
    c, drops, cp = _pack(tables)
    counts = c if counts is None else np.asarray(counts, np.int32)
    radius, w = (np.ascontiguousarray(weights[0], np.int32), np.ascontiguousarray(weights[1], np.float32))
    msg = ctypes.create_string_buffer(256)
    n_work = ctypes.c_int64(-1)
    rc = emu.rr_emu_lens_check(len(tables), H, W, counts.ctypes.data, drops.ctypes.data, cp if cap is None else cap, len(radius),
                               radius.ctypes.data, w.ctypes.data, msg, 256, ctypes.byref(n_work))
    return rc, msg.value.decode(), n_work.value


# ---- arithmetic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", lc.SCENES)
def test_gxx_build_equals_the_numpy_statement(emu, name, dtype):
    img, tabs, want, want_alpha = lc.scene(name, dtype)
    got, alpha = _emu_apply(emu, np.array(img), tabs, lc.WEIGHTS)
    assert got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))                   # float32: bit for bit; bytes: byte for byte
    assert np.array_equal(alpha.view(np.uint32), want_alpha.view(np.uint32))
    assert np.array_equal(got[:, :, :, :][np.broadcast_to(want_alpha[:, None] == 0, got.shape)],
                          img[np.broadcast_to(want_alpha[:, None] == 0, img.shape)])   # A == 0: the input
    # the scene does what it is there for: drops change pixels, partial coverage exists, the empty frame is untouched
    assert (want != img).any() and ((want_alpha > 0) & (want_alpha < 1)).any() and (want_alpha == 1).any()
    if name == 'odd':
        assert np.array_equal(want[1], img[1]) and not want_alpha[1].any()
        assert (want_alpha[2] > 0).mean() > 0.5                                      # the drop wider than the frame


def test_statement_properties():
    """What the model promises, on the statement itself: a drop of coverage 1 with mag 1, radius 0 and rim 0 shows the image rotated by
    180 degrees about its centre where the refraction gain is 1 (the centre pixel), radius 0 is the single tap 1, weights sum to 1."""
    for s in (0.5, 1.2, 5.0):
        R, w = lens.gaussian_class(s)
        assert R == min(int(np.ceil(3 * s)), 15) and len(w) == 2 * R + 1 and w.dtype == np.float32
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6 and np.array_equal(w, w[::-1])
    assert lens.gaussian_class(0.0)[0] == 0 and lens.gaussian_class(0.0)[1][0] == 1.0
    img = lc.images(1, 21, 21, np.float32)
    t = np.zeros(1, lens.LENS_DROP_DTYPE)
    t[0] = (10.0, 10.0, 6.0, 6.0, 1.0, 0.01, 0.0, 0)
    out, alpha = lens.apply_numpy(img, [t], lens.blur_table([0.0]), alpha=True)
    assert alpha[0, 10, 10] == 1.0 and np.array_equal(out[0, :, 10, 10], img[0, :, 10, 10])
    assert alpha[0, 0, 0] == 0.0 and np.array_equal(out[0, :, 0, :], img[0, :, 0, :])
    # one pixel off the centre the sample lies a little more than one pixel on the other side (g > 1): between pixels 9 and 8
    lo, hi = np.minimum(img[0, :, 10, 8], img[0, :, 10, 9]), np.maximum(img[0, :, 10, 8], img[0, :, 10, 9])
    assert ((out[0, :, 10, 11] >= lo) & (out[0, :, 10, 11] <= hi)).all()


# ---- the library's checks of a batch (rr_lens.h check_frame, check_classes) --------------------------------------------
def test_the_checks_accept_the_scenes_and_count_the_work(emu):
    rc, msg, n_work = _emu_check(emu, lc.TABLES, lc.H, lc.W)
    assert rc == 0 and msg == '' and n_work == 8 + 4
    rc, msg, n_work = _emu_check(emu, lc.WIDE_TABLES, lc.WIDE_H, lc.WIDE_W)
    assert rc == 0 and n_work == 3 * 2


def _bad_tables():
    """(name, table, match) for every refusal of a record, on the 61 x 47 frame."""
    good = lc.FRAME0[6].copy()
    out = []
    for field, value, match in (('cx', np.nan, 'finite'), ('cy', np.inf, 'finite'), ('rx', 0.0, 'positive'), ('ry', -1.0, 'positive'),
                                ('rx', np.nan, 'finite'), ('mag', 0.99, 'mag'), ('mag', np.inf, 'finite'), ('edge', 0.0, 'edge'),
                                ('edge', 1.001, 'edge'), ('rim', -0.01, 'rim'), ('rim', 1.5, 'rim'), ('sigma_class', 3.0, 'class'),
                                ('sigma_class', 0.5, 'class'), ('sigma_class', -1.0, 'class'), ('sigma_class', np.nan, 'finite')):
        t = np.array([good])
        t[0][field] = value
        out.append(('%s=%r' % (field, value), t, match))
    # two boxes that share one pixel column / row; and a pair that only touches in x but not in y is fine
    a, b = good.copy(), good.copy()
    a['cx'], a['cy'], a['rx'], a['ry'] = 10.0, 10.0, 3.0, 3.0          # box x 7 .. 14, y 7 .. 14
    b['cx'], b['cy'], b['rx'], b['ry'] = 18.0, 17.0, 3.5, 3.0          # box x 14 .. 22, y 14 .. 21: shares pixel (14, 14)
    out.append(('overlap', np.array([a, b]), 'overlap'))
    return out


def test_the_checks_refuse_what_the_header_lists(emu):
    for name, t, match in _bad_tables():
        rc, msg, _ = _emu_check(emu, [t], lc.H, lc.W)
        assert rc == RR_E_ARG and match in msg, (name, rc, msg)
        with pytest.raises(ValueError):
            lens.check_table(t, lc.H, lc.W, 3)
    # boxes one pixel apart are accepted
    t = _bad_tables()[-1][1].copy()
    t[1]['cx'] = 19.0                                                  # box x 15 .. 23
    assert _emu_check(emu, [t], lc.H, lc.W)[0] == 0
    lens.check_table(t, lc.H, lc.W, 3)
    # counts and the blur table
    assert _emu_check(emu, [lc.FRAME0], lc.H, lc.W, cap=4)[0] == RR_E_ARG                          # count above cap
    many = np.repeat(lc.FRAME0[:1], 129)
    assert 'count' in _emu_check(emu, [many], lc.H, lc.W)[1]                                       # above RR_MAX_LENS_DROPS
    assert _emu_check(emu, [lc.FRAME0], lc.H, lc.W, counts=[-1])[0] == RR_E_ARG
    for radius in ([16], [-1], [0] * 17, []):
        assert _emu_check(emu, [lc.FRAME0[:0]], lc.H, lc.W, weights=(radius, lc.WEIGHTS[1]))[0] == RR_E_ARG, radius
    w = lc.WEIGHTS[1].copy()
    w[2, 30] = np.nan
    assert _emu_check(emu, [lc.FRAME0[:0]], lc.H, lc.W, weights=(lc.WEIGHTS[0], w))[0] == RR_E_ARG
    w[2, 30], w[1, 30] = 0.1, np.nan                                   # beyond class 1's 9 taps: not read
    assert _emu_check(emu, [lc.FRAME0[:0]], lc.H, lc.W, weights=(lc.WEIGHTS[0], w))[0] == 0


# ---- the generator -------------------------------------------------------------------------------------------------
GEN = dict(count=40, radius=(2, 12), life_s=(0.5, 3.0), hz=10, seed=11)


def _boxes(L, t):
    return [lens.drop_box(d, L.H, L.W) for d in t]


def test_table_is_a_pure_function_of_seed_and_frame():
    a, b = lens.LensDrops(96, 160, **GEN), lens.LensDrops(96, 160, **GEN)
    for k in (0, 7, 123, 2 ** 31):
        assert a.table(k).tobytes() == b.table(k).tobytes() == a.table(k).tobytes()
    b.table(5)
    assert a.table(7).tobytes() == b.table(7).tobytes()                # no state between calls
    other = lens.LensDrops(96, 160, **dict(GEN, seed=12))
    assert a.table(7).tobytes() != other.table(7).tobytes()
    assert a.weights()[0].dtype == np.int32 and a.weights()[1].shape == (16, 31) and a.weights()[1].dtype == np.float32


def test_kept_boxes_are_disjoint_and_kept_drops_stay():
    L = lens.LensDrops(96, 160, **GEN)
    n_cls = len(L.weights()[0])
    prev = None
    lives_seen, counts = set(), []
    for k in range(200):
        rec, born, kept = L.slots(k)
        g, born2 = L.lives(k)
        assert np.array_equal(born, born2)
        t = L.table(k)
        assert t.tobytes() == rec[kept].tobytes() and len(t) <= lens.RR_MAX_LENS_DROPS and len(t) <= L.count
        counts.append(len(t))
        lens.check_table(t, L.H, L.W, n_cls)                           # ranges, classes, pairwise disjoint boxes
        bx = _boxes(L, t)
        assert all(not lens.boxes_overlap(bx[i], bx[j]) for i in range(len(bx)) for j in range(i))
        assert (t['ry'] >= t['rx']).all() and (t['rx'] >= np.float32(2)).all() and (t['rx'] <= np.float32(12)).all()
        assert (t['sigma_class'] == np.floor(t['sigma_class'])).all() and t['sigma_class'].max(initial=0) < n_cls
        if prev is not None:
            pg, prec, pkept = prev
            same_life = pg == g
            # within a life nothing changes; a new life of the same slot is a new drop
            assert prec[same_life].tobytes() == rec[same_life].tobytes()
            assert all(prec[j].tobytes() != rec[j].tobytes() for j in np.nonzero(~same_life)[0])
            # a drop kept at k - 1 and alive at k is kept at k, with identical record bytes
            assert kept[pkept & same_life].all()
        lives_seen.update((j, float(g[j])) for j in range(L.count))
        prev = (g, rec, kept)
    assert len(lives_seen) > 3 * L.count                               # lives did turn over in the 200 frames
    assert min(counts) > 0 and len(set(counts)) > 1


def test_for_view_gives_other_tables():
    L = lens.LensDrops(96, 160, **GEN)
    a, b = L.for_view(0), L.for_view(1)
    assert (a.H, a.W, a.count, a.radius, a.hz) == (L.H, L.W, L.count, L.radius, L.hz)
    assert a.table(3).tobytes() != b.table(3).tobytes() != L.table(3).tobytes()
    assert a.table(3).tobytes() == L.for_view(0).table(3).tobytes()
    assert np.array_equal(a.weights()[1], L.weights()[1])


# ---- arguments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(count=129), dict(count=-1), dict(radius=(0, 4)), dict(radius=(5, 4)), dict(aspect=(0.9, 1.2)),
                                dict(mag=(0.5, 2)), dict(blur=(-1, 2)), dict(edge=(0.0, 0.4)), dict(edge=(0.1, 1.1)), dict(rim=(-0.1, 0.5)),
                                dict(rim=(0.2, 1.2)), dict(life_s=(0, 5)), dict(hz=0), dict(hz=float('nan')), dict(seed=1.5),
                                dict(radius=3), dict(mag=(3, float('inf')))])
def test_bad_ranges_are_value_errors(kw):
    with pytest.raises(ValueError):
        lens.LensDrops(96, 160, **kw)


def test_other_argument_errors():
    with pytest.raises(ValueError):
        lens.LensDrops(0, 160)
    L = lens.LensDrops(96, 160, **GEN)
    for k in (-1, 1.5, True):
        with pytest.raises(ValueError):
            L.table(k)
    with pytest.raises(ValueError):
        L.for_view(-1)
    img = lc.images(1, lc.H, lc.W, np.uint8)
    with pytest.raises(ValueError):
        lens.apply_numpy(img, [], lc.WEIGHTS)                          # one table per image
    with pytest.raises(ValueError):
        lens.apply_numpy(img.astype(np.float64), [lc.FRAME0], lc.WEIGHTS)
    with pytest.raises(ValueError):
        lens.apply_numpy(img, [lc.FRAME0], (lc.WEIGHTS[0], lc.WEIGHTS[1][:, :5]))
    with pytest.raises(ValueError):
        lens.blur_table([1.0] * 17)


def test_size_mismatch_with_the_augmenter(tmp_path_factory):
    torch = pytest.importorskip('torch')                               # (augment.py imports torch; the CPU tier has it)
    augment = importlib.import_module('rain-rendering_amd.augment')
    root = str(tmp_path_factory.mktemp('lensdb'))
    h.synthetic.write_streak_db(os.path.join(root, 'rainstreakdb'))
    kw = dict(streaks_db=os.path.join(root, 'rainstreakdb'), sequence='data_object/training')
    with pytest.raises(ValueError, match='375 x 1242'):
        augment.RainAugment('kitti', lens=lens.LensDrops(96, 160), **kw)
    with pytest.raises(TypeError):
        augment.RainAugment('kitti', lens='drops', **kw)
    with pytest.raises(ValueError, match='return_lens_alpha'):
        augment.RainAugment('kitti', return_lens_alpha=True, **kw)
    aug = augment.RainAugment('kitti', lens=lens.LensDrops(375, 1242, count=5), return_lens_alpha=True, **kw)
    assert aug.lens.count == 5 and aug.frame_size() == (375, 1242)
    la = augment.LensAugment(lens.LensDrops(96, 160))
    with pytest.raises(ValueError, match='96 x 160'):
        la(torch.zeros((1, 3, 95, 160), dtype=torch.uint8), [0])
    with pytest.raises(TypeError):
        la(torch.zeros((1, 3, 96, 160), dtype=torch.float64), [0])
    with pytest.raises(ValueError, match='on the GPU'):
        la(torch.zeros((1, 3, 96, 160), dtype=torch.uint8), [0])
    with pytest.raises(TypeError):
        augment.LensAugment('drops')


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_abi_layout(built):
    lib = h.hb.load_library()
    assert lib.rr_sizeof_lens_drop() == 32 == h.hb.LENS_DROP_DTYPE.itemsize == lens.LENS_DROP_DTYPE.itemsize
    assert h.hb.LENS_DROP_DTYPE == lens.LENS_DROP_DTYPE
    assert lib.rr_sizeof_lens_batch() == ctypes.sizeof(h.hb.rr_lens_batch) == 80
    offs = {name: getattr(h.hb.rr_lens_batch, name).offset for name, _ in h.hb.rr_lens_batch._fields_}
    assert offs == dict(n=0, H=4, W=8, dtype=12, images=16, out=24, alpha_out=32, counts=40, drops=48, cap=56, n_classes=60,
                        class_radius=64, weights=72)
    assert [n for n in lens.LENS_DROP_DTYPE.names] == ['cx', 'cy', 'rx', 'ry', 'mag', 'edge', 'rim', 'sigma_class']
    assert h.hb.RR_MAX_LENS_DROPS == lens.RR_MAX_LENS_DROPS == 128
    assert lib.rr_version() == 400
    assert lib.rr_lens_drops_device(None, None, None) == RR_E_ARG          # no context: refused, not a crash
