"""CPU tier of the rain layer as a file: the ABI of rr_pipeline_set_layer_png; the pixel's statement
(tools/layer_png.py encode / decode) against the g++ build of csrc/rr_layer.h layer_rgba (tests/hostemu/layer_png_emu.cpp), byte for
byte, and the derived round-trip bound; the tEXt chunk of rr_io_write_frames_text and imgops.png_from_scanlines(text=); and the
driver's --rain_layer around a stand-in for the GPU context: which buffers reach which slot, and what the files hold."""
import ctypes
import importlib
import os

import numpy as np
import pytest
from PIL import Image

import helpers as h
import test_driver_host as tdh

hb = h.hb
main_mod = tdh.main_mod
imgops = tdh.imgops
lp = importlib.import_module('rain-rendering_amd.tools.layer_png')


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(importlib.import_module('__graft_entry__').build_emu('layerpngemu'))
    lib.rr_emu_layer_rgba.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.rr_emu_layer_rgba.restype = None
    lib.rr_emu_layer_rows.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.rr_emu_layer_rows.restype = None
    return lib


def _emu_encode(emu, layer):
    layer = np.ascontiguousarray(layer, np.float32)
    out = np.full(layer.shape, 77, np.uint8)
    emu.rr_emu_layer_rgba(layer.size // 4, layer.ctypes.data, out.ctypes.data)
    return out


def _inside(rng, n):
    """n random float32 pixels that meet the condition 0 <= T <= 1, 0 <= L_c <= 1 - T (in float64, on the float32 values)."""
    T = rng.random(n).astype(np.float32)
    T[: n // 8] = rng.choice(np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -30, 0.5], np.float32), n // 8)
    a = 1.0 - T.astype(np.float64)
    L = (rng.random((n, 3)) * a[:, None]).astype(np.float32)
    L[: n // 16] = (a[: n // 16, None] * np.ones(3)).astype(np.float32)          # L == a: the colour clamp's edge
    L = np.minimum(L.astype(np.float64), a[:, None])
    L32 = L.astype(np.float32)
    L32 = np.where(L32.astype(np.float64) > a[:, None], np.nextafter(L32, np.float32(0)), L32)
    return np.concatenate([L32, T[:, None]], axis=1)


def _condition(layer):
    L, T = layer[..., :3].astype(np.float64), layer[..., 3].astype(np.float64)
    return bool(((T >= 0) & (T <= 1)).all() and ((L >= 0) & (L <= (1 - T)[..., None])).all())


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_abi_of_the_arming_call(built):
    lib = hb.load_library()
    assert lib.rr_sizeof_pipeline_layer_png() == ctypes.sizeof(hb.rr_pipeline_layer_png) == 24
    assert lib.rr_version() == 400
    # the existing structs keep their sizes
    assert lib.rr_sizeof_pipeline_lens() == 64 and lib.rr_sizeof_layer_out() == 16 and lib.rr_sizeof_frame_out() == 72
    assert lib.rr_sizeof_pipeline_layer() == ctypes.sizeof(hb.rr_pipeline_layer) == 16


# ---- the statement, twice --------------------------------------------------------------------------------------------
def test_g_plus_plus_build_equals_numpy_inside_the_condition(built, emu):
    g = np.linspace(0.0, 1.0, 52, dtype=np.float32)
    T, f = np.meshgrid(g, g, indexing='ij')
    a = np.float32(1.0) - T
    grid = np.stack([a * f, a * f * np.float32(0.5), a * (np.float32(1.0) - f), T], axis=-1).astype(np.float32)
    rnd = _inside(np.random.default_rng(11), 20000)
    for layer in (grid, rnd):
        want = lp.encode(layer)
        assert want.dtype == np.uint8 and want.shape == layer.shape
        assert np.array_equal(_emu_encode(emu, layer), want)
    assert len(np.unique(lp.encode(rnd)[:, 3])) == 256             # every alpha code is met


def test_g_plus_plus_build_equals_numpy_outside_the_condition(built, emu):
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 2 ** 32, (40000, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)      # any bit pattern: NaN, inf, denormals
    mid = (rng.random((40000, 4)) * 4.0 - 2.0).astype(np.float32)  # T < 0, T > 1, L < 0, L > a
    mid[::7, 3] = rng.random(mid[::7].shape[0]).astype(np.float32)
    special = np.array([[np.nan, 0.1, 0.2, 0.5], [0.1, np.nan, 0.2, np.nan], [np.inf, -np.inf, 0.3, 0.2], [0.1, 0.2, 0.3, -np.inf],
                        [0.1, 0.2, 0.3, np.inf], [-0.0, -1.0, 5.0, 0.25], [1e30, 1e-30, -1e-30, 0.999]], np.float32)
    with np.errstate(all='ignore'):
        for layer in (bits, mid, special):
            assert not _condition(layer)
            assert np.array_equal(_emu_encode(emu, layer), lp.encode(layer))
    assert np.array_equal(lp.encode(special[1:2])[0], [0, 0, 0, 0])          # NaN alpha -> 0 -> a transparent pixel
    assert np.array_equal(lp.encode(special[0:1])[0, [2, 3]], [0, 128])      # NaN colour -> 0; 127.5 -> 128 (even)


def test_alpha_products_exactly_on_a_half(built, emu):
    """a * 255.0f == k + 0.5 in float32: found by search around (k + 0.5) / 255, for odd and even k."""
    found = {}
    for k in list(range(0, 12)) + [62, 63, 126, 127, 128, 200, 253, 254]:
        c = np.float32((k + 0.5) / 255.0)
        cand = c
        for _ in range(8):
            cand = np.nextafter(cand, np.float32(0))
        for _ in range(17):
            if cand * np.float32(255.0) == np.float32(k + 0.5) and np.float32(1.0) - (np.float32(1.0) - cand) == cand:
                found[k] = cand
                break
            cand = np.nextafter(cand, np.float32(2))
    assert any(k % 2 for k in found) and any(k % 2 == 0 for k in found) and len(found) >= 6, found
    for k, a in found.items():
        T = np.float32(1.0) - a
        assert np.float32(1.0) - T == a                            # the pixel's own a is the one searched for
        px = np.array([[0.0, 0.0, 0.0, T]], np.float32)
        want = k if k % 2 == 0 else k + 1                          # half to even
        assert lp.encode(px)[0, 3] == want == _emu_encode(emu, px)[0, 3], (k, a)


def test_the_two_ends(built, emu):
    clear = np.array([[0.0, 0.0, 0.0, 1.0]], np.float32)
    assert np.array_equal(lp.encode(clear), [[0, 0, 0, 0]]) and np.array_equal(_emu_encode(emu, clear), [[0, 0, 0, 0]])
    opaque = np.array([[0.25, 0.5, 1.0, 0.0]], np.float32)
    for got in (lp.encode(opaque), _emu_encode(emu, opaque)):
        assert np.array_equal(got, [[255, 128, 64, 255]])          # file order R G B A of the layer's B G R; 63.75 -> 64, 127.5 -> 128
    lb, lg, lr, t = lp.decode(np.array([[255, 128, 64, 255]], np.uint8))
    assert t[0] == 0.0 and (lb[0], lg[0], lr[0]) == (64 / 255, 128 / 255, 1.0)
    with pytest.raises(ValueError):
        lp.encode(np.zeros((2, 4), np.float64))
    with pytest.raises(ValueError):
        lp.decode(np.zeros((2, 3), np.uint8))


def test_round_trip_within_the_derived_bound():
    """decode(encode(x)) for every pixel of random layers that meet the condition: no exclusions; the condition is asserted on the
    inputs alone.  BOUND = 1/510 + 2^-17 / 255 + 2^-25 (+ 2^-48): tools/layer_png.py, DESIGN 5r."""
    assert abs(lp.BOUND - (1 / 510 + 2.0 ** -17 / 255 + 2.0 ** -25)) < 1e-14
    worst = 0.0
    for seed in (1, 2, 3):
        layer = _inside(np.random.default_rng(seed), 200000)
        assert _condition(layer)
        dec = lp.decode(lp.encode(layer))
        for c in range(4):
            worst = max(worst, float(np.abs(dec[c] - layer[:, c].astype(np.float64)).max()))
        x = np.random.default_rng(seed + 10).random(len(layer))
        for c in range(3):
            got, want = dec[3] * x + dec[c], layer[:, 3].astype(np.float64) * x + layer[:, c].astype(np.float64)
            assert float(np.abs(got - want).max()) <= 2 * lp.BOUND
    print('round trip: max error %.9g, bound %.9g' % (worst, lp.BOUND))
    assert worst <= lp.BOUND
    assert worst > 0.9 / 510                                       # (the bound is met nearly: it is not slack)


def test_sub_filter_of_the_two_statements(built, emu):
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (3, 1), (5, 7), (4, 33)):
        rgba = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        rows = np.zeros((H, 1 + 4 * W), np.uint8)
        emu.rr_emu_layer_rows(H, W, rgba.ctypes.data, rows.ctypes.data)
        assert np.array_equal(rows, lp.sub_filter(rgba))
        back = np.cumsum(rows[:, 1:].reshape(H, W, 4).astype(np.int64), axis=1) % 256
        assert (rows[:, 0] == 1).all() and np.array_equal(back.astype(np.uint8), rgba)


# ---- the text chunk --------------------------------------------------------------------------------------------------
def _chunks(path):
    data = open(path, 'rb').read()
    out, at = [], 8
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], 'big')
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def test_write_frames_text(tmp_path, built):
    rng = np.random.default_rng(3)
    n, H, W = 3, 6, 9
    rgba = rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8)
    stride = (H * (1 + 4 * W) + 15) // 16 * 16
    block = np.zeros((n, stride), np.uint8)
    for k in range(n):
        block[k, :H * (1 + 4 * W)] = lp.sub_filter(rgba[k]).ravel()
    texts = [repr(0.1 * (k + 1) - 0.2) for k in range(n)]
    paths = [str(tmp_path / ('t%d.png' % k)) for k in range(n)]
    paths[1] = None                                                # (a skipped frame)
    st = hb.io_write_frames_text(paths, block, W, H, 'rain-shift', texts)
    assert not st.any() and not os.path.exists(str(tmp_path / 't1.png'))
    for k in (0, 2):
        with Image.open(paths[k]) as im:
            assert im.mode == 'RGBA' and np.array_equal(np.array(im), rgba[k]) and im.text == {'rain-shift': texts[k]}
        assert [c[0] for c in _chunks(paths[k])] == [b'IHDR', b'tEXt', b'IDAT', b'IEND']
        bgr = np.zeros((H, W, 3), np.uint8)
        assert hb.load_library().rr_png_read_bgr8(os.fsencode(paths[k]), bgr.ctypes.data, H, W) == 0
        assert np.array_equal(bgr, rgba[k][..., 2::-1])
        layer, shift = imgops.read_rain_layer(paths[k])
        assert shift == float(texts[k]) and repr(shift) == texts[k]
        dec = lp.decode(rgba[k])
        assert layer.shape == (H, W, 4) and all(np.array_equal(layer[..., c], dec[c]) for c in range(4))
    # texts == NULL: byte for byte rr_io_write_frames
    plain = [str(tmp_path / ('p%d.png' % k)) for k in range(n)]
    ref = [str(tmp_path / ('r%d.png' % k)) for k in range(n)]
    assert not hb.io_write_frames_text(plain, block, W, H).any()
    assert not hb.io_write_frames(ref, None, block, None, W, H).any()
    for a, b in zip(plain, ref):
        assert open(a, 'rb').read() == open(b, 'rb').read()
    assert imgops.read_rain_layer(plain[0])[1] is None
    # png_from_scanlines(text=) writes the same file as the native call (the library's own encoder is the default strategy)
    for k in (0, 2):
        q = str(tmp_path / ('g%d.png' % k))
        imgops.png_from_scanlines(q, block[k, :H * (1 + 4 * W)], W, H, strategy=3, text=('rain-shift', texts[k]))
        assert open(q, 'rb').read() == open(paths[k], 'rb').read()
        imgops.png_from_scanlines(q, block[k, :H * (1 + 4 * W)], W, H)
        assert open(q, 'rb').read() == open(ref[k], 'rb').read()


def test_a_bad_keyword_is_refused(tmp_path, built):
    H, W = 2, 2
    block = np.zeros((1, 48), np.uint8)
    block[0, :H * (1 + 4 * W)] = lp.sub_filter(np.zeros((H, W, 4), np.uint8)).ravel()
    p = str(tmp_path / 'k.png')
    for kw in ('', 'x' * 80, ' lead', 'trail ', 'two  spaces', 'tab\tinside', 'del\x7f', 'c1\x85'):
        with pytest.raises(ValueError):
            hb.io_write_frames_text([p], block, W, H, kw, ['1.0'])
        with pytest.raises(ValueError):
            imgops.png_from_scanlines(p, block[0, :H * (1 + 4 * W)], W, H, text=(kw, '1.0'))
        assert not os.path.exists(p)
    lib = hb.load_library()
    status = np.zeros(1, np.int32)
    pp, keep = hb._c_paths([p])
    tp = (ctypes.c_char_p * 1)(b'1.0')
    assert lib.rr_io_write_frames_text(1, pp, block.ctypes.data, 48, W, H, None, tp, 1, status.ctypes.data) == -1      # RR_E_ARG: no keyword
    assert not os.path.exists(p)
    for kw in ('x' * 79, 'Latin-1 \xe9\xff', 'rain-shift'):
        assert not hb.io_write_frames_text([p], block, W, H, kw, ['1.0']).any()
        with Image.open(p) as im:
            assert im.text == {kw: '1.0'}


# ---- the driver ------------------------------------------------------------------------------------------------------
class LayerContext(tdh.RecordingContext):
    """RecordingContext that records what rr_pipeline_set_layer_png / rr_pipeline_set_layer get and which submit they precede, and
    "renders" layer rows and shifts that name the frame (its image's first pixel).  The armed state is cleared by a submit, so a submit
    without a fresh arming call shows."""
    armed, png, lay = None, None, None

    def __init__(self, device=0):
        super().__init__(device)
        self._out = {}

    def pipeline_set_layer_png(self, slot, bufs, H=0, W=0):
        LayerContext.png = None if bufs is None else dict(slot=slot, bufs=bufs, H=H, W=W)

    def pipeline_set_layer(self, slot, outs):
        LayerContext.lay = None if outs is None else dict(slot=slot, outs=outs)

    def pipeline_submit_prepared(self, slot, prep, n=None):
        n_ = prep.n if n is None else n
        self._out[slot] = (LayerContext.png, LayerContext.lay)
        LayerContext.armed.append(dict(slot=slot, n=n_, png=LayerContext.png, lay=LayerContext.lay))
        LayerContext.png = LayerContext.lay = None
        super().pipeline_submit_prepared(slot, prep, n)

    def pipeline_wait(self, slot):
        prep, n = self.batches.get(slot, (None, 0))
        firsts = [np.array(tdh._frame_inputs(prep.frames[k])[0])[0, 0] for k in range(n)] if prep is not None else []
        ok = super().pipeline_wait(slot)
        png, lay = self._out.pop(slot, (None, None))
        for k in range(n if png is not None else 0):
            H, W = png['H'], png['W']
            rows = np.zeros((H, 1 + 4 * W), np.uint8)              # filter type 0 rows: every pixel names the frame
            rows[:, 1:] = np.tile(np.array([firsts[k][0], firsts[k][1], firsts[k][2], 200], np.uint8), W)
            png['bufs'][k][...] = rows.ravel()
            lay['outs'][k]['shift'][0] = _shift_of(firsts[k])
        return ok


def _shift_of(first):
    return (int(first[0]) - 100) / 7.0 + int(first[1]) / 300.0     # (a double whose repr has 17 digits)


def _run(tmp, src, out_name, native, monkeypatch, extra, batch=3):
    monkeypatch.setenv('RAIN_BATCH', str(batch))
    monkeypatch.setenv('RAIN_NATIVE_IO', '1' if native else '0')
    monkeypatch.setattr(hb, 'RainHip', LayerContext)
    tdh.RecordingContext.log = []
    LayerContext.armed, LayerContext.png, LayerContext.lay = [], None, None
    argv = ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', os.path.join(tmp, 'rainstreakdb'),
            '-i', '5', '--output', os.path.join(tmp, out_name), '--noverbose']
    gen = main_mod.main(argv + list(extra))
    return gen, LayerContext.armed, os.path.join(tmp, out_name, 'kitti', 'data_object', 'training', 'rain', '5mm')


def test_the_flag():
    assert main_mod._parse(['--dataset', 'kitti']).rain_layer is False
    assert main_mod._parse(['--dataset', 'kitti', '--rain_layer']).rain_layer is True


@pytest.mark.parametrize("native", [True, False])
def test_a_run_arms_every_batch_and_writes_each_frames_own_layer(tmp_path, built, monkeypatch, native):
    tmp = str(tmp_path)
    n = 8
    src, img_dir, dep_dir = tdh._dataset(tmp, n)
    with open(os.path.join(dep_dir, '%06d.png' % 2), 'wb') as fh:   # frame 2 is skipped in its batch: the gap is closed
        fh.write(b'not a png')
    gen, armed, out = _run(tmp, src, 'out', native, monkeypatch, ['--rain_layer'])
    assert (gen.timing[0].get('route') == 'native') == native
    assert sum(s['n'] for s in armed) == n - 1
    for sub in armed:
        png, lay = sub['png'], sub['lay']
        assert png is not None and lay is not None and png['slot'] == lay['slot'] == sub['slot'] and (png['H'], png['W']) == (48, 80)
        assert len(png['bufs']) == len(lay['outs']) == sub['n']
        assert all(b.dtype == np.uint8 and b.size == 48 * (1 + 4 * 80) for b in png['bufs'])
        assert all(o['layer'] is None and o['shift'].dtype == np.float64 and o['shift'].size == 1 for o in lay['outs'])
    for i in range(n):
        p = os.path.join(out, 'rain_layer', '%06d.png' % i)
        assert os.path.exists(p) == (i != 2)
        if i == 2:
            continue
        first = imgops.imread_bgr(os.path.join(img_dir, '%06d.png' % i))[0, 0]
        with Image.open(p) as im:
            rgba = np.array(im)
            assert im.text == {'rain-shift': repr(_shift_of(first))}
        assert rgba.shape == (48, 80, 4) and (rgba == np.array([first[0], first[1], first[2], 200], np.uint8)).all()   # its own frame's rows
        layer, shift = imgops.read_rain_layer(p)
        assert shift == _shift_of(first)
        assert os.path.exists(os.path.join(out, 'rainy_image', '%06d.png' % i)) and os.path.exists(os.path.join(out, 'rain_mask', '%06d.png' % i))


def test_both_routes_write_the_same_files(tmp_path, built, monkeypatch):
    tmp = str(tmp_path)
    src, _, _ = tdh._dataset(tmp, 4)
    _, _, out_n = _run(tmp, src, 'out_n', True, monkeypatch, ['--rain_layer'])
    _, _, out_g = _run(tmp, src, 'out_g', False, monkeypatch, ['--rain_layer'])
    for i in range(4):
        for sub in ('rain_layer', 'rainy_image', 'rain_mask'):
            a, b = (os.path.join(o, sub, '%06d.png' % i) for o in (out_n, out_g))
            assert open(a, 'rb').read() == open(b, 'rb').read(), (sub, i)


def test_no_flag_arms_nothing_and_writes_no_layer(tmp_path, built, monkeypatch):
    tmp = str(tmp_path)
    src, _, _ = tdh._dataset(tmp, 3)
    for native in (True, False):
        gen, armed, out = _run(tmp, src, 'out%d' % native, native, monkeypatch, [])
        assert len(armed) == 1 and all(s['png'] is None and s['lay'] is None for s in armed)
        assert not os.path.exists(os.path.join(out, 'rain_layer'))
    # the files of a run with the flag are those of the run without it
    _, _, out_f = _run(tmp, src, 'out_flag', True, monkeypatch, ['--rain_layer'])
    for i in range(3):
        for sub in ('rainy_image', 'rain_mask'):
            a, b = (os.path.join(o, sub, '%06d.png' % i) for o in (out, out_f))
            assert open(a, 'rb').read() == open(b, 'rb').read()


def test_device_particles_and_lens_flags_go_with_it(tmp_path, built, monkeypatch):
    tmp = str(tmp_path)
    src, _, _ = tdh._dataset(tmp, 3)
    gen, armed, out = _run(tmp, src, 'out', True, monkeypatch, ['--rain_layer', '--device_particles'])
    assert all(s['png'] is not None for s in armed) and len(os.listdir(os.path.join(out, 'rain_layer'))) == 3


def test_skip_keeps_its_rule(tmp_path, built, monkeypatch):
    """--conflict_strategy skip: a frame is skipped when its rainy or mask file exists; a layer file alone does not make it one."""
    tmp = str(tmp_path)
    src, _, _ = tdh._dataset(tmp, 4)
    out = os.path.join(tmp, 'out', 'kitti', 'data_object', 'training', 'rain', '5mm')
    for sub, name in (('rainy_image', '000000.png'), ('rain_mask', '000001.png'), ('rain_layer', '000002.png')):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
        with open(os.path.join(out, sub, name), 'wb') as fh:
            fh.write(b'old')
    gen, armed, out = _run(tmp, src, 'out', True, monkeypatch, ['--rain_layer', '--conflict_strategy', 'skip'])
    assert sorted(os.path.basename(s['file']) for s in gen.stats) == ['000002.png', '000003.png']
    assert sorted(os.listdir(os.path.join(out, 'rain_layer'))) == ['000002.png', '000003.png']
    with open(os.path.join(out, 'rain_layer', '000002.png'), 'rb') as fh:
        assert fh.read(4) == b'\x89PNG'                            # written anew
