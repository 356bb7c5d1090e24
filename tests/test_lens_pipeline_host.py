"""CPU tier of the drops on the lens inside the frame pipeline: the ABI of rr_pipeline_set_lens; the label's statement
(tools/lens.py alpha_label); LensDrops.from_spec; the g++ build of the interleaved chain (tests/hostemu/lens_hwc_emu.cpp: the addressing
of k_lens_drops_hwc over csrc/rr_lens.h) against apply_numpy through a transpose, byte for byte; and the driver's flags around a stand-in
for the GPU context: which tables reach which slot, in which order."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

import helpers as h
import lens_cases as lc
import test_driver_host as tdh

lens = lc.lens
hb = h.hb
main_mod = tdh.main_mod


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_abi_of_the_arming_call(built):
    lib = hb.load_library()
    assert lib.rr_sizeof_pipeline_lens() == ctypes.sizeof(hb.rr_pipeline_lens) == 64
    assert hb.RR_TENSOR_U8_HWC == 3 and (hb.RR_TENSOR_U8, hb.RR_TENSOR_F32) == (0, 1)
    # the existing structs keep their sizes (tests/test_abi.py pins the numbers; here: the binding still agrees with the library)
    for fn, st in (('rr_sizeof_frame_in', hb.rr_frame_in), ('rr_sizeof_frame_out', hb.rr_frame_out), ('rr_sizeof_prepass_in', hb.rr_prepass_in),
                   ('rr_sizeof_prepass_out', hb.rr_prepass_out), ('rr_sizeof_tensor_batch', hb.rr_tensor_batch),
                   ('rr_sizeof_lens_batch', hb.rr_lens_batch), ('rr_sizeof_camera', hb.rr_camera)):
        assert getattr(lib, fn)() == ctypes.sizeof(st), fn
    assert lib.rr_sizeof_lens_batch() == 80 and lib.rr_sizeof_lens_drop() == 32 and lib.rr_sizeof_frame_out() == 72


# ---- the label -----------------------------------------------------------------------------------------------------
def test_alpha_label():
    a = np.array([0.0, 1.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 3.5 / 255, 0.2, 0.999], np.float32)
    v = lens.alpha_label(a)
    assert v.dtype == np.uint8 and v.shape == a.shape
    assert v[0] == 0 and v[1] == 255
    # half to even wherever the float32 product is exactly x.5
    for x, got in zip(a[2:6], v[2:6]):
        p = np.float32(x) * np.float32(255.0)
        want = int(np.rint(p))
        assert got == want
        if p == np.floor(p) + np.float32(0.5):
            assert got % 2 == 0
    exact = np.array([0.5, 1.5, 2.5, 126.5], np.float32) / np.float32(255.0)
    prod = exact * np.float32(255.0)
    halves = prod == np.floor(prod) + np.float32(0.5)
    assert halves.any()                                          # the case exists in float32
    assert (lens.alpha_label(exact)[halves] % 2 == 0).all()
    assert np.array_equal(lens.alpha_label(np.array([[0.25]], np.float64)), np.array([[64]], np.uint8))     # 63.75 -> 64
    assert lens.alpha_label(np.float32(0.5)) == 128              # 127.5 -> 128 (even)


# ---- from_spec -----------------------------------------------------------------------------------------------------
def test_from_spec(tmp_path):
    L = lens.LensDrops.from_spec('12,3', 40, 60, 10)
    assert (L.H, L.W, L.count, L.seed, L.hz) == (40, 60, 12, 3, 10.0)
    assert lens.LensDrops.from_spec('7', 40, 60, 25).seed == 0 and lens.LensDrops.from_spec(' 7 ', 40, 60, 25).hz == 25.0
    p = tmp_path / 'lens.json'
    p.write_text(json.dumps(dict(count=5, radius=[2, 9], life_s=[0.3, 0.5])))
    L = lens.LensDrops.from_spec(str(p), 40, 60, 20)
    assert (L.count, L.radius, L.life_s, L.hz, L.seed) == (5, (2.0, 9.0), (0.3, 0.5), 20.0, 0)
    ref = lens.LensDrops(40, 60, count=5, radius=(2, 9), life_s=(0.3, 0.5), hz=20)
    assert all(np.array_equal(L.table(k), ref.table(k)) for k in range(4))
    p.write_text(json.dumps(dict(count=5, hz=30, seed=4)))
    L = lens.LensDrops.from_spec(str(p), 40, 60, 20)
    assert L.hz == 30.0 and L.seed == 4                          # the file's own rate wins
    bad = tmp_path / 'bad.json'
    for text in ('{not json', '[1, 2]', json.dumps(dict(count=5, H=3)), json.dumps(dict(colour='red')), json.dumps(dict(count=500)),
                 json.dumps(dict(radius=[5, 2]))):
        bad.write_text(text)
        with pytest.raises(ValueError):
            lens.LensDrops.from_spec(str(bad), 40, 60, 10)
    for spec in ('', 'abc', '12,', ',3', '12,3,4', '1.5', '-3', '129', '12;3', str(tmp_path / 'missing.json')):
        with pytest.raises(ValueError):
            lens.LensDrops.from_spec(spec, 40, 60, 10)


# ---- the interleaved chain under g++ -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def emu(built):
    lib = ctypes.CDLL(os.path.join(h.ROOT, 'tests', 'hostemu', 'liblenshwcemu.so'))
    lib.rr_emu_lens_hwc_apply.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 2 + [ctypes.c_void_p] * 2
    return lib


@pytest.mark.parametrize("name", ['odd', 'wide'])
def test_interleaved_chain_equals_the_statement(emu, name):
    img, tabs, want, want_alpha = lc.scene(name, 'uint8')
    n, _, H, W = img.shape
    hwc = np.ascontiguousarray(img.transpose(0, 2, 3, 1))
    counts = np.array([len(t) for t in tabs], np.int32)
    cap = max(1, int(counts.max()))
    drops = np.zeros((n, cap), lens.LENS_DROP_DTYPE)
    for f, t in enumerate(tabs):
        drops[f, :len(t)] = t
    radius, w = lens.check_weights(lc.WEIGHTS)
    out = np.full_like(hwc, 7)
    label = np.full((n, H, W), 9, np.uint8)
    rc = emu.rr_emu_lens_hwc_apply(n, H, W, hwc.ctypes.data, out.ctypes.data, label.ctypes.data, counts.ctypes.data, drops.ctypes.data, cap,
                                   len(radius), radius.ctypes.data, w.ctypes.data)
    assert rc == 0
    assert np.array_equal(out.transpose(0, 3, 1, 2), want)       # byte for byte
    assert np.array_equal(label, lens.alpha_label(want_alpha))
    assert (want != img).any() and ((label > 0) & (label < 255)).any() and (label == 255).any()
    untouched = np.broadcast_to((want_alpha == 0)[..., None], hwc.shape)
    assert np.array_equal(out[untouched], hwc[untouched])
    # without the label
    out2 = np.zeros_like(hwc)
    assert emu.rr_emu_lens_hwc_apply(n, H, W, hwc.ctypes.data, out2.ctypes.data, None, counts.ctypes.data, drops.ctypes.data, cap, len(radius),
                                     radius.ctypes.data, w.ctypes.data) == 0
    assert np.array_equal(out2, out)


# ---- the driver ----------------------------------------------------------------------------------------------------
class LensContext(tdh.RecordingContext):
    """RecordingContext that also records what rr_pipeline_set_lens gets and which submit it precedes, and "renders" label rows
    that name the slot position.  (The armed state is cleared by a submit here, so a submit without a fresh arming call shows.)"""
    armed, state = None, None

    def __init__(self, device=0):
        super().__init__(device)
        self._alpha = {}

    def pipeline_set_lens(self, slot, tables, weights=None, H=0, W=0, alpha_png=None):
        LensContext.state = dict(slot=slot, tables=None if tables is None else [np.array(t) for t in tables], weights=weights, H=H, W=W,
                                 alpha_png=alpha_png)

    def pipeline_submit_prepared(self, slot, prep, n=None):
        n_ = prep.n if n is None else n
        st = LensContext.state
        self._alpha[slot] = None if st is None else st['alpha_png']
        LensContext.armed.append(dict(slot=slot, n=n_, lens=st, bgs=[np.array(tdh._frame_inputs(prep.frames[k])[0]) for k in range(n_)]))
        LensContext.state = None
        super().pipeline_submit_prepared(slot, prep, n)

    def pipeline_wait(self, slot):
        n = self.batches.get(slot, (None, 0))[1]
        ok = super().pipeline_wait(slot)
        for k in range(n if self._alpha.get(slot) is not None else 0):
            rows = np.zeros((self.H, 1 + 4 * self.W), np.uint8)   # filter type 0 rows
            rows[:, 1:] = np.tile(np.array([k + 1, k + 1, k + 1, 255], np.uint8), self.W)
            self._alpha[slot][k][...] = rows.ravel()
        return ok


def _base(tmp, src, out_name):
    return ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', os.path.join(tmp, 'rainstreakdb'),
            '-i', '5', '--output', os.path.join(tmp, out_name), '--noverbose']


def _run(tmp, src, out_name, native, monkeypatch, extra, batch=3):
    monkeypatch.setenv('RAIN_BATCH', str(batch))
    monkeypatch.setenv('RAIN_NATIVE_IO', '1' if native else '0')
    monkeypatch.setattr(hb, 'RainHip', LensContext)
    tdh.RecordingContext.log = []
    LensContext.armed, LensContext.state = [], None
    gen = main_mod.main(_base(tmp, src, out_name) + list(extra))
    return gen, LensContext.armed, os.path.join(tmp, out_name, 'kitti', 'data_object', 'training', 'rain', '5mm')


def test_flags_and_their_refusals(tmp_path, built):
    ns = main_mod._parse(['--dataset', 'kitti'])
    assert ns.lens_drops is None and ns.lens_alpha is False
    ns = main_mod._parse(['--dataset', 'kitti', '--lens_drops', '12,3', '--lens_alpha'])
    assert ns.lens_drops == '12,3' and ns.lens_alpha is True
    assert main_mod._lens(ns) is ns
    for argv, match in ((['--lens_alpha'], 'needs --lens_drops'), (['--lens_drops', 'abc'], 'COUNT'), (['--lens_drops', '200'], 'at most'),
                        (['--lens_drops', '12,3,4'], 'COUNT'), (['--lens_drops', ''], 'COUNT'), (['--lens_drops', '-1'], 'count'),
                        (['--lens_drops', str(tmp_path / 'none.json')], 'COUNT')):
        with pytest.raises(SystemExit, match=match):
            main_mod._lens(main_mod._parse(['--dataset', 'kitti'] + argv))
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps(dict(edge=[0.5, 2.0])))
    with pytest.raises(SystemExit, match='edge'):
        main_mod._lens(main_mod._parse(['--dataset', 'kitti', '--lens_drops', str(bad)]))
    # the flags need no particular particle route
    for extra in ([], ['--device_particles'], ['--device_particles', '--particle_model', 'field']):
        main_mod._lens(main_mod._parse(['--dataset', 'kitti', '--lens_drops', '5'] + extra))


@pytest.mark.parametrize("native", [True, False])
def test_a_run_arms_every_batch_with_its_frames_tables(tmp_path, built, monkeypatch, native):
    tmp = str(tmp_path)
    n = 8
    src, img_dir, dep_dir = tdh._dataset(tmp, n)
    with open(os.path.join(dep_dir, '%06d.png' % 2), 'wb') as fh:   # frame 2 is skipped in its batch: the tables close the gap like the inputs
        fh.write(b'not a png')
    spec = tmp_path / 'lens.json'
    spec.write_text(json.dumps(dict(count=12, radius=[2, 8], life_s=[0.2, 0.4], seed=5)))
    gen, armed, out = _run(tmp, src, 'out', native, monkeypatch, ['--lens_drops', str(spec), '--lens_alpha'])
    assert (gen.timing[0].get('route') == 'native') == native
    L = lens.LensDrops(48, 80, count=12, radius=(2, 8), life_s=(0.2, 0.4), seed=5, hz=10)       # KITTI: 10 Hz
    tabs = [L.table(i) for i in range(n)]
    assert len({t.tobytes() for t in tabs}) > 1 and all(len(t) >= 4 for t in tabs)
    imgops = tdh.imgops
    ident = {imgops.imread_bgr(os.path.join(img_dir, '%06d.png' % i)).tobytes(): i for i in range(n)}
    seen = []
    for sub in armed:
        st = sub['lens']
        assert st is not None and st['slot'] == sub['slot'] and (st['H'], st['W']) == (48, 80) and len(st['tables']) == sub['n']
        assert st['weights'][0].tobytes() == L.weights()[0].tobytes() and st['weights'][1].tobytes() == L.weights()[1].tobytes()
        assert st['alpha_png'] is not None and len(st['alpha_png']) == sub['n'] and all(a.size == 48 * (1 + 4 * 80) for a in st['alpha_png'])
        for k in range(sub['n']):
            i = ident[sub['bgs'][k].tobytes()]                     # the frame that sits in slot position k
            assert st['tables'][k].tobytes() == tabs[i].tobytes(), (i, k)
            seen.append(i)
    assert sorted(seen) == [i for i in range(n) if i != 2]
    from PIL import Image
    for i in range(n):
        p = os.path.join(out, 'lens_alpha', '%06d.png' % i)
        assert os.path.exists(p) == (i != 2)
        if i != 2:
            assert np.array(Image.open(p)).shape == (48, 80, 4)
            assert os.path.exists(os.path.join(out, 'rainy_image', '%06d.png' % i)) and os.path.exists(os.path.join(out, 'rain_mask', '%06d.png' % i))


def test_no_flag_arms_nothing_and_writes_no_label(tmp_path, built, monkeypatch):
    tmp = str(tmp_path)
    src, _, _ = tdh._dataset(tmp, 3)
    gen, armed, out = _run(tmp, src, 'out', True, monkeypatch, [])
    assert len(armed) == 1 and all(s['lens'] is None for s in armed)
    assert not os.path.exists(os.path.join(out, 'lens_alpha'))
    gen, armed, out = _run(tmp, src, 'out2', True, monkeypatch, ['--lens_drops', '6'])
    assert all(s['lens'] is not None and s['lens']['alpha_png'] is None for s in armed)
    assert not os.path.exists(os.path.join(out, 'lens_alpha'))


def test_rig_view_wears_its_own_lens(tmp_path, built, monkeypatch):
    tmp = str(tmp_path)
    src, img_dir, _ = tdh._dataset(tmp, 3)
    import shutil
    shutil.rmtree(os.path.join(tmp, 'particles'))
    gen, armed, out = _run(tmp, src, 'out', True, monkeypatch,
                           ['--lens_drops', '10,2', '--device_particles', '--particle_model', 'rig', '--rig', 'stereo:0.54', '--rig_view', '1'])
    L = lens.LensDrops(48, 80, count=10, seed=2, hz=10).for_view(1)
    plain = lens.LensDrops(48, 80, count=10, seed=2, hz=10)
    ident = {tdh.imgops.imread_bgr(os.path.join(img_dir, '%06d.png' % i)).tobytes(): i for i in range(3)}
    n_seen = 0
    for sub in armed:
        for k in range(sub['n']):
            i = ident[sub['bgs'][k].tobytes()]
            assert sub['lens']['tables'][k].tobytes() == L.table(i).tobytes()
            n_seen += 1
    assert n_seen == 3 and any(L.table(i).tobytes() != plain.table(i).tobytes() for i in range(3))


def test_skip_keeps_its_rule(tmp_path, built, monkeypatch):
    """--conflict_strategy skip: a frame is skipped when its rainy or mask file exists; a label file alone does not make it one."""
    tmp = str(tmp_path)
    n = 4
    src, _, _ = tdh._dataset(tmp, n)
    out = os.path.join(tmp, 'out', 'kitti', 'data_object', 'training', 'rain', '5mm')
    for sub, name in (('rainy_image', '000000.png'), ('rain_mask', '000001.png'), ('lens_alpha', '000002.png')):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
        with open(os.path.join(out, sub, name), 'wb') as fh:
            fh.write(b'old')
    gen, armed, out = _run(tmp, src, 'out', True, monkeypatch, ['--lens_drops', '6', '--lens_alpha', '--conflict_strategy', 'skip'])
    assert sorted(os.path.basename(s['file']) for s in gen.stats) == ['000002.png', '000003.png']
    L = lens.LensDrops(48, 80, count=6, hz=10)
    got = [t.tobytes() for sub in armed for t in sub['lens']['tables']]
    assert sorted(got) == sorted(L.table(i).tobytes() for i in (2, 3))       # the sequence's own indices, not positions in the work list
    with open(os.path.join(out, 'lens_alpha', '000002.png'), 'rb') as fh:
        assert fh.read(4) == b'\x89PNG'                          # written anew
