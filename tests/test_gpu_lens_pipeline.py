"""GPU tier of the drops on the lens inside the frame pipeline (rr_pipeline_set_lens, k_lens_drops_hwc, k_png_alpha).

Kernel alone
  1. rr_lens_drops_device with RR_TENSOR_U8_HWC == the numpy statement (tools/lens.py apply_numpy) on the scenes of tests/lens_cases.py,
     with and without alpha_out, on a non-default torch stream; rr_augment_frames_device refuses the layout.
Pipeline parity (one set-up: a 96 x 160 scene with 150 streaks, six frames as three batches of two on the three slots, each armed with
its frames' tables of L = LensDrops(96, 160, count=12, radius=(2, 12), life_s=(0.2, 0.4), seed=0))
  2. image_u8 == apply_numpy of the unarmed run's image_u8, byte for byte; mask, mask_i32 and status are the unarmed run's;
  3. rainy_png / mask_png / alpha_png as scanlines and entropy-coded (RR_OPT_PNG_DEFLATE), written by rr_io_write_frames, read back;
  4. a disarmed slot gives the unarmed bytes again; an armed slot 0 is honoured by pipeline_frames.
Errors and re-submit
  5. every RR_E_ARG of rr_pipeline_set_lens, RR_E_STATE on a busy slot, a submit with the wrong n or frame size;
  6. arena regrowth: the re-submitted batch wears its drops once.
Driver
  7. main.py --device_particles --lens_drops <json> --lens_alpha against the same command without the flags;
  8. the same frames through RainAugment(lens=L, return_lens_alpha=True); the XML particle route;
  9. RAIN_NATIVE_IO=0 writes the same three files per frame."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import helpers as h
import lens_cases as lc
import test_gpu_edge_cases as edge
import test_gpu_prepass as tp
from test_gpu_augment import DEV, streaks_db          # noqa: F401  (streaks_db: a fixture)
from test_gpu_driver import _make_dataset
from test_gpu_pipeline_async import _defocused_frames
from test_lens_host import _bad_tables, _pack

pytestmark = pytest.mark.gpu

lens = lc.lens
hb = h.hb
imgops = importlib.import_module('rain-rendering_amd.common.imgops')
augment = importlib.import_module('rain-rendering_amd.augment')
main_mod = importlib.import_module('rain-rendering_amd.main')
RR_E_ARG, RR_E_STATE = -1, -4
H, W = 96, 160
L_KW = dict(count=12, radius=(2, 12), life_s=(0.2, 0.4), seed=0)


def _statement(images_hwc, tables, weights):
    """apply_numpy on interleaved frames [n, H, W, 3]: (images with the drops, the byte label)."""
    planar = np.ascontiguousarray(np.asarray(images_hwc).transpose(0, 3, 1, 2))
    out, alpha = lens.apply_numpy(planar, tables, weights, alpha=True)
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1)), lens.alpha_label(alpha), alpha


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rh(built):
    ctx = hb.RainHip(0)
    yield ctx
    ctx.close()


def _run_hwc(rh, img, tabs, want_alpha, stream=None):
    n, _, h_, w_ = img.shape
    d_img = torch.from_numpy(np.ascontiguousarray(np.asarray(img).transpose(0, 2, 3, 1))).to(DEV)
    d_out = torch.full_like(d_img, 3)
    d_alpha = torch.full((n, h_, w_), -1.0, dtype=torch.float32, device=DEV) if want_alpha else None
    torch.cuda.synchronize()
    rh.lens_drops_device(d_img.data_ptr(), d_out.data_ptr(), n, h_, w_, False, tabs, lc.WEIGHTS,
                         alpha_ptr=None if d_alpha is None else d_alpha.data_ptr(), stream=stream, layout='hwc')
    return d_out, d_alpha


@pytest.mark.parametrize("name", ['odd', 'wide'])
def test_interleaved_bytes_equal_the_statement(rh, name):
    img, tabs, want, want_alpha = lc.scene(name, 'uint8')
    want_hwc = want.transpose(0, 2, 3, 1)
    d_out, d_alpha = _run_hwc(rh, img, tabs, True)
    got, alpha = d_out.cpu().numpy(), d_alpha.cpu().numpy()
    diff = np.argwhere(got != want_hwc)
    print('%s: %d of %d bytes differ' % (name, len(diff), want.size), diff[:5].tolist())
    assert np.array_equal(got, want_hwc)
    assert np.array_equal(alpha.view(np.uint32), want_alpha.view(np.uint32))
    keep = np.broadcast_to((alpha == 0)[..., None], got.shape)
    assert np.array_equal(got[keep], img.transpose(0, 2, 3, 1)[keep]) and keep.any() and not keep.all()
    d_out2, none = _run_hwc(rh, img, tabs, False)                      # no alpha asked for: the same bytes
    assert none is None and np.array_equal(d_out2.cpu().numpy(), want_hwc)
    s = torch.cuda.Stream(DEV)                                        # the caller's stream, read back on it
    with torch.cuda.stream(s):
        d_out3, d_alpha3 = _run_hwc(rh, img, tabs, True, stream=s.cuda_stream)
        got3, alpha3 = d_out3.cpu().numpy(), d_alpha3.cpu().numpy()
    assert np.array_equal(got3, want_hwc) and np.array_equal(alpha3.view(np.uint32), want_alpha.view(np.uint32))


def test_augment_frames_refuses_the_interleaved_layout(rh):
    b = hb.rr_tensor_batch()
    img = torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device=DEV)
    dep = torch.ones((1, 8, 8), dtype=torch.float32, device=DEV)
    out, mask = torch.zeros_like(img), torch.zeros_like(dep)
    sims, fog = np.zeros(1, hb.SIM_FRAME_DTYPE), np.zeros(4)
    b.n, b.H, b.W, b.dtype = 1, 8, 8, hb.RR_TENSOR_U8_HWC
    b.images, b.depth, b.sims, b.fog, b.drops_cap = img.data_ptr(), dep.data_ptr(), sims.ctypes.data, fog.ctypes.data, 16
    b.rainy_out, b.mask_out = out.data_ptr(), mask.data_ptr()
    torch.cuda.synchronize()
    assert rh.lib.rr_augment_frames_device(rh.h, ctypes.byref(b), None) == RR_E_ARG
    assert rh.lib.rr_last_error(rh.h).decode().startswith('rr_augment_frames_device')


# ---- 2 .. 4. pipeline parity ---------------------------------------------------------------------------------------
class _Pipe:
    """The shared set-up: context, six frames, the unarmed run, L's tables and the statement's results (computed once)."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.sc = sc = h.Scene(tmp, H, W, 150, n_frames=6, seed0=31)
        self.rh = rh = hb.RainHip(0)
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        rh.set_colormap(imgops.viridis_lut())
        consts, We = tp._setup(rh, H, W, 25)
        self.frames = []
        for i in range(6):
            bg, depth = tp._scene(H, W, 31 + i)
            self.frames.append(dict(bg_u8=(bg * 255).astype(np.uint8), depth=depth.astype(np.float32), fog=consts, omega=sc.omega,
                                    drops=sc.product_drops(i)))
        self.L = lens.LensDrops(H, W, **L_KW)
        self.tables = [self.L.table(i) for i in range(6)]
        self.row = H * (1 + 4 * W)
        self.ref = self.run(None)
        ref_img = np.stack([o['image_u8'] for o in self.ref['outs']])
        self.want, self.want_label, self.want_alpha = _statement(ref_img, self.tables, self.L.weights())
        for a in (self.want, self.want_label):
            a.setflags(write=False)

    def outs(self, png):
        o = [dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W)), mask_i32=np.zeros((H, W), np.int32),
                  status=np.zeros(len(self.frames[i]['drops']), np.int32)) for i in range(6)]
        blocks = None
        if png:
            blocks = [self.rh.host_rows(6, (self.row,), np.uint8) for _ in range(3)]
            for i in range(6):
                o[i]['rainy_png'], o[i]['mask_png'] = blocks[0][1][i], blocks[1][1][i]
        return o, blocks

    def run(self, tables, png=False, alpha=False, armed_slots=(0, 1, 2)):
        """Three batches of two on the three slots, all in flight together; slot s armed with tables[2 s : 2 s + 2] (None: never armed)."""
        rh = self.rh
        o, blocks = self.outs(png)
        for slot in range(3):
            if tables is not None and slot in armed_slots:
                a = [blocks[2][1][2 * slot + k] for k in range(2)] if alpha else None
                rh.pipeline_set_lens(slot, tables[2 * slot:2 * slot + 2], self.L.weights(), H, W, alpha_png=a)
            rh.pipeline_submit(slot, self.frames[2 * slot:2 * slot + 2], o[2 * slot:2 * slot + 2])
        for slot in range(3):
            assert rh.pipeline_wait(slot)
        for slot in range(3):
            rh.pipeline_set_lens(slot, None)
        return dict(outs=o, blocks=blocks)

    def free(self, res):
        for b in res['blocks'] or ():
            self.rh.host_free(b[0])


@pytest.fixture(scope='module')
def pipe(built, tmp_path_factory):
    p = _Pipe(tmp_path_factory.mktemp('lenspipe'))
    yield p
    p.rh.close()


def test_the_setup_shows_drops(pipe):
    shown = [len(t) for t in pipe.tables]
    print('drops shown per frame:', shown)
    assert all(n >= 8 for n in shown)                                 # an empty table cannot pass the parity tests
    assert len({t.tobytes() for t in pipe.tables}) == 6
    boxes = [lens.drop_box(d, H, W) for t in pipe.tables for d in t]
    assert any(b[2] == 0 for b in boxes) and any(b[3] == H - 1 for b in boxes)      # clipped at the top and the bottom edge


def test_armed_slots_equal_the_statement(pipe):
    got = pipe.run(pipe.tables)
    for i, (o, r) in enumerate(zip(got['outs'], pipe.ref['outs'])):
        diff = np.argwhere(o['image_u8'] != pipe.want[i])
        print('frame %d: %d of %d bytes differ from the statement, %d from the unarmed run' %
              (i, len(diff), pipe.want[i].size, int((o['image_u8'] != r['image_u8']).sum())), diff[:4].tolist())
        assert np.array_equal(o['image_u8'], pipe.want[i]), i
        assert not np.array_equal(o['image_u8'], r['image_u8']), i
        for k in ('mask', 'mask_i32', 'status'):
            assert np.array_equal(o[k], r[k]), (i, k)
        assert r['mask'].max() > 0


@pytest.mark.parametrize("deflate", [0, 1])
def test_png_payloads(pipe, deflate, tmp_path):
    rh = pipe.rh
    rh.set_option(hb.RR_OPT_PNG_DEFLATE, deflate)
    try:
        plain = pipe.run(None, png=True)
        got = pipe.run(pipe.tables, png=True, alpha=True)
    finally:
        rh.set_option(hb.RR_OPT_PNG_DEFLATE, 0)
    names = {}
    for tag, res, kinds in (('u', plain, 2), ('a', got, 3)):
        for k, kind in enumerate(('rainy', 'mask', 'label')[:kinds]):
            names[tag, kind] = [str(tmp_path / ('%s_%s_%d.png' % (tag, kind, i))) for i in range(6)]
        st = hb.io_write_frames(names[tag, 'rainy'], names[tag, 'mask'], res['blocks'][0][0], res['blocks'][1][0], W, H)
        assert not st.any()
        if kinds == 3:
            assert not hb.io_write_frames(names[tag, 'label'], None, res['blocks'][2][0], None, W, H).any()
    for i in range(6):
        if deflate:
            for b in got['blocks']:
                assert b[1][i][:4].tobytes() == b'RRZ1', i            # entropy-coded on the device, the label too
        img = np.array(Image.open(names['a', 'rainy'][i]))
        assert img.shape == (H, W, 4) and (img[..., 3] == 255).all()
        assert np.array_equal(img[..., :3], pipe.want[i]), i
        assert np.array_equal(img[..., :3], got['outs'][i]['image_u8']), i
        assert open(names['a', 'mask'][i], 'rb').read() == open(names['u', 'mask'][i], 'rb').read(), i
        assert np.array_equal(np.array(Image.open(names['u', 'rainy'][i]))[..., :3], pipe.ref['outs'][i]['image_u8']), i
        lab = np.array(Image.open(names['a', 'label'][i]))
        assert lab.shape == (H, W, 4) and (lab[..., 3] == 255).all()
        for c in range(3):
            assert np.array_equal(lab[..., c], pipe.want_label[i]), (i, c)
        assert (pipe.want_label[i] == 255).any() and ((pipe.want_label[i] > 0) & (pipe.want_label[i] < 255)).any()
    pipe.free(plain)
    pipe.free(got)


def test_disarming_and_the_synchronous_call(pipe):
    rh = pipe.rh
    # armed once, then disarmed (run() disarms every slot when it is done): the unarmed bytes again
    again = pipe.run(None)
    for o, r in zip(again['outs'], pipe.ref['outs']):
        assert np.array_equal(o['image_u8'], r['image_u8'])
    # only slot 1 armed: its two frames wear drops, the others do not
    mixed = pipe.run(pipe.tables, armed_slots=(1,))
    for i, (o, r) in enumerate(zip(mixed['outs'], pipe.ref['outs'])):
        assert np.array_equal(o['image_u8'], pipe.want[i] if i in (2, 3) else r['image_u8']), i
    # rr_pipeline_frames runs on slot 0
    rh.pipeline_set_lens(0, pipe.tables[:2], pipe.L.weights(), H, W)
    try:
        sync = rh.pipeline_frames(pipe.frames[:2], want_mask_i32=True)
    finally:
        rh.pipeline_set_lens(0, None)
    for i in range(2):
        assert np.array_equal(sync[i]['image_u8'], pipe.want[i]) and np.array_equal(sync[i]['mask_i32'], pipe.ref['outs'][i]['mask_i32'])
    sync = rh.pipeline_frames(pipe.frames[:2], want_mask_i32=True)
    assert np.array_equal(sync[1]['image_u8'], pipe.ref['outs'][1]['image_u8'])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def _lens_arg(tabs, h_, w_, weights=lc.WEIGHTS, cap=None, counts=None, n=None):
    c, drops, cp = _pack(tabs)
    counts = c if counts is None else np.asarray(counts, np.int32)
    radius, w = np.ascontiguousarray(weights[0], np.int32), np.ascontiguousarray(weights[1], np.float32)
    b = hb.rr_pipeline_lens()
    b.n, b.H, b.W, b.cap = len(tabs) if n is None else n, h_, w_, cp if cap is None else cap
    b.counts, b.drops = counts.ctypes.data, drops.ctypes.data
    b.n_classes, b.class_radius, b.weights = len(radius), radius.ctypes.data, w.ctypes.data
    return b, (counts, drops, radius, w)


def test_refusals(pipe):
    rh = pipe.rh
    lib, hnd = rh.lib, rh.h

    def rc_of(slot, b_keep):
        return lib.rr_pipeline_set_lens(hnd, slot, ctypes.byref(b_keep[0]))

    def refused(what, b_keep, slot=2):
        assert rc_of(slot, b_keep) == RR_E_ARG, what
        assert lib.rr_last_error(hnd).decode().startswith('rr_pipeline_set_lens'), what

    good = [lc.FRAME0]
    for name, t, _ in _bad_tables():                                  # every field, overlapping boxes among them
        refused(name, _lens_arg([t], lc.H, lc.W))
    refused('slot -1', _lens_arg(good, lc.H, lc.W), slot=-1)
    refused('slot 3', _lens_arg(good, lc.H, lc.W), slot=3)
    refused('n = 0', _lens_arg(good, lc.H, lc.W, n=0))
    refused('H = 0', _lens_arg(good, 0, lc.W))
    refused('W < 0', _lens_arg(good, lc.H, -5))
    refused('count above cap', _lens_arg(good, lc.H, lc.W, cap=4))
    refused('count above RR_MAX_LENS_DROPS', _lens_arg([np.repeat(lc.FRAME0[:1], 129)], lc.H, lc.W))
    refused('negative count', _lens_arg(good, lc.H, lc.W, counts=[-1]))
    refused('radius 16', _lens_arg(good, lc.H, lc.W, weights=([0, 4, 16], lc.WEIGHTS[1])))
    refused('no class', _lens_arg(good, lc.H, lc.W, weights=([], lc.WEIGHTS[1])))
    w = lc.WEIGHTS[1].copy()
    w[2, 3] = np.inf
    refused('a weight that is not finite', _lens_arg(good, lc.H, lc.W, weights=(lc.WEIGHTS[0], w)))
    b, keep = _lens_arg(good, lc.H, lc.W)
    b.counts = None
    refused('null counts', (b, keep))
    # nothing changed: slot 2 is still unarmed, a batch on it gives the unarmed bytes
    o, _ = pipe.outs(False)
    rh.pipeline_submit(2, pipe.frames[4:6], o[4:6])
    # ... and while it is in flight the slot cannot be armed
    assert rc_of(2, _lens_arg(pipe.tables[4:6], H, W, weights=pipe.L.weights())) == RR_E_STATE
    assert lib.rr_pipeline_set_lens(hnd, 2, None) == RR_E_STATE
    assert rh.pipeline_wait(2)
    assert np.array_equal(o[4]['image_u8'], pipe.ref['outs'][4]['image_u8']) and np.array_equal(o[5]['image_u8'], pipe.ref['outs'][5]['image_u8'])
    # a submit that does not match the armed batch is refused with nothing enqueued
    try:
        rh.pipeline_set_lens(1, pipe.tables[:1], pipe.L.weights(), H, W)                    # one frame armed, two submitted
        o, _ = pipe.outs(False)
        with pytest.raises(RuntimeError, match='armed'):
            rh.pipeline_submit(1, pipe.frames[:2], o[:2])
        rh.pipeline_set_lens(1, pipe.tables[:2], pipe.L.weights(), H + 1, W)                # another frame size
        with pytest.raises(RuntimeError, match='armed'):
            rh.pipeline_submit(1, pipe.frames[:2], o[:2])
        assert rh.pipeline_wait(1) and not o[0]['image_u8'].any()                           # the slot is idle, nothing was written
        rh.pipeline_set_lens(1, pipe.tables[:2], pipe.L.weights(), H, W)                    # the next good batch is correct
        rh.pipeline_submit(1, pipe.frames[:2], o[:2])
        assert rh.pipeline_wait(1)
        assert np.array_equal(o[0]['image_u8'], pipe.want[0]) and np.array_equal(o[1]['image_u8'], pipe.want[1])
        # a batch that renders nothing (the pre-pass alone runs on slot 0)
        rh.pipeline_set_lens(0, pipe.tables[:2], pipe.L.weights(), H, W)
        with pytest.raises(RuntimeError, match='renders nothing'):
            rh.prepass_frames([dict(bg=f['bg_u8'] / 255.0, depth=f['depth'], fog=f['fog']) for f in pipe.frames[:2]])
    finally:
        for s in range(3):
            rh.pipeline_set_lens(s, None)


# ---- 6. arena regrowth ---------------------------------------------------------------------------------------------
def test_resubmit_after_arena_regrowth_wears_the_drops_once(tmp_path, built):
    sc = h.Scene(tmp_path, edge.H, edge.W, 0, frames=_defocused_frames(420))
    bg, env = sc.frame_inputs(0)
    drops = sc.product_drops(0)
    fr = dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=drops)
    L = lens.LensDrops(edge.H, edge.W, **L_KW)
    tab = L.table(0)
    assert len(tab) >= 8
    rh = hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)

        def out():
            return dict(image_u8=np.zeros((edge.H, edge.W, 3), np.uint8), mask=np.zeros((edge.H, edge.W)),
                        mask_i32=np.zeros((edge.H, edge.W), np.int32), status=np.zeros(len(drops), np.int32))
        armed, plain = out(), out()
        rh.pipeline_set_lens(0, [tab], L.weights(), edge.H, edge.W)
        rh.pipeline_submit(0, [fr], [armed])
        assert rh.pipeline_wait(0) is False                         # the first wait reports the regrowth
        rh.pipeline_submit(0, [fr], [armed])                        # the armed state is still on the slot
        assert rh.pipeline_wait(0) is True
        rh.pipeline_set_lens(0, None)
        rh.pipeline_submit(0, [fr], [plain])
        assert rh.pipeline_wait(0) is True
        want, _, _ = _statement(plain['image_u8'][None], [tab], L.weights())
        assert np.array_equal(armed['image_u8'], want[0])           # the statement applied ONCE to the unarmed image
        assert not np.array_equal(armed['image_u8'], plain['image_u8'])
        twice, _, _ = _statement(want, [tab], L.weights())
        assert not np.array_equal(twice[0], want[0])                # (twice would show)
        for k in ('mask', 'mask_i32', 'status'):
            assert np.array_equal(armed[k], plain[k]), k
    finally:
        rh.close()


# ---- 7 .. 9. the driver --------------------------------------------------------------------------------------------
def _spec(tmp):
    p = os.path.join(tmp, 'lens.json')
    with open(p, 'w') as f:
        json.dump(dict(count=L_KW['count'], radius=list(L_KW['radius']), life_s=list(L_KW['life_s']), seed=L_KW['seed']), f)
    return p


def _drive(tmp, src, streaks, out_name, extra, monkeypatch, native=True, rate='5'):
    monkeypatch.setenv('RAIN_NATIVE_IO', '1' if native else '0')
    monkeypatch.setenv('RAIN_BATCH', '2')                             # two batches, a ragged last one
    gen = main_mod.main(['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', streaks, '-i', rate,
                         '--output', os.path.join(tmp, out_name), '--noverbose'] + list(extra))
    assert len(gen.stats) == 3
    return gen, os.path.join(tmp, out_name, 'kitti', 'data_object', 'training', 'rain', rate + 'mm')


def _rgb(path):
    a = np.array(Image.open(path))
    assert a.shape[2] == 4 and (a[..., 3] == 255).all()
    return a[..., :3]


def _check_against_plain(out_lens, out_plain, L, n=3):
    """Every rainy file == apply_numpy of the plain run's file with L.table(i); the label files are the statement's; the mask files
    are byte-identical."""
    plain = np.stack([_rgb(os.path.join(out_plain, 'rainy_image', '%06d.png' % i)) for i in range(n)])
    tables = [L.table(i) for i in range(n)]
    assert all(len(t) >= 8 for t in tables)
    want, label, _ = _statement(plain, tables, L.weights())
    for i in range(n):
        got = _rgb(os.path.join(out_lens, 'rainy_image', '%06d.png' % i))
        print('frame %d: %d bytes differ from the statement' % (i, int((got != want[i]).sum())))
        assert np.array_equal(got, want[i]) and not np.array_equal(got, plain[i]), i
        a = open(os.path.join(out_lens, 'rain_mask', '%06d.png' % i), 'rb').read()
        assert a == open(os.path.join(out_plain, 'rain_mask', '%06d.png' % i), 'rb').read() and len(a) > 300, i
        lab = np.array(Image.open(os.path.join(out_lens, 'lens_alpha', '%06d.png' % i)))
        assert lab.shape == plain[i].shape[:2] + (4,) and (lab[..., 3] == 255).all()
        assert all(np.array_equal(lab[..., c], label[i]) for c in range(3)), i


KH, KW = 375, 1242                                         # KITTI's frames: the device's particle generator renders the sensor's size


@pytest.fixture(scope='module')
def kitti_runs(built, tmp_path_factory, streaks_db):
    """One KITTI-sized tree of three frames, rendered twice with --device_particles: with the lens flags and without."""
    tmp = str(tmp_path_factory.mktemp('lensdriver'))
    src = os.path.join(tmp, 'source')
    h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), 3, KH, KW, depth_m=None)
    spec = _spec(tmp)
    with pytest.MonkeyPatch.context() as mp:
        gen, out_lens = _drive(tmp, src, streaks_db, 'lens', ['--device_particles', '--lens_drops', spec, '--lens_alpha'], mp, rate='25')
        assert gen.timing[0].get('route') == 'native'
        _, out_plain = _drive(tmp, src, streaks_db, 'plain', ['--device_particles'], mp, rate='25')
    return dict(src=src, out_lens=out_lens, out_plain=out_plain, L=lens.LensDrops(KH, KW, hz=10, **L_KW))


def test_driver_device_particles(kitti_runs):
    assert not os.path.exists(os.path.join(kitti_runs['out_plain'], 'lens_alpha'))
    _check_against_plain(kitti_runs['out_lens'], kitti_runs['out_plain'], kitti_runs['L'])


def test_driver_xml_route_and_general_route(tmp_path, built, monkeypatch):
    """No --device_particles (the particle file's drops, packed by the host): lens drops all the same; and RAIN_NATIVE_IO=0, the
    general route, writes the same three files per frame as the native one."""
    tmp = str(tmp_path)
    src, xml = _make_dataset(tmp)
    streaks = os.path.join(tmp, 'rainstreakdb')
    spec = _spec(tmp)
    gen, out_lens = _drive(tmp, src, streaks, 'lens', ['--lens_drops', spec, '--lens_alpha'], monkeypatch)
    assert gen.timing[0].get('route') == 'native'
    _, out_plain = _drive(tmp, src, streaks, 'plain', [], monkeypatch)
    _check_against_plain(out_lens, out_plain, lens.LensDrops(96, 160, hz=10, **L_KW))
    gen_g, out_gen = _drive(tmp, src, streaks, 'general', ['--lens_drops', spec, '--lens_alpha'], monkeypatch, native=False)
    assert gen_g.timing[0].get('route') != 'native'
    for i in range(3):
        for kind in ('rainy_image', 'rain_mask', 'lens_alpha'):
            a = open(os.path.join(out_lens, kind, '%06d.png' % i), 'rb').read()
            b = open(os.path.join(out_gen, kind, '%06d.png' % i), 'rb').read()
            assert a == b and len(a) > 200, (kind, i)


def test_driver_equals_rain_augment(kitti_runs, streaks_db):
    """The driver's three frames == RainAugment(lens=L, return_lens_alpha=True) on uint8 at frame_index = i."""
    n, L, out = 3, kitti_runs['L'], kitti_runs['out_lens']
    img_dir = os.path.join(kitti_runs['src'], 'kitti', 'data_object', 'training', 'image_2')
    rgb = np.stack([np.array(Image.open(os.path.join(img_dir, '%06d.png' % i)).convert('RGB')) for i in range(n)])
    depth = np.stack([np.array(Image.open(os.path.join(img_dir, 'depth', '%06d.png' % i))).astype(np.float32) / 256. for i in range(n)])
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', lens=L, return_lens_alpha=True)
    try:
        rainy, mask, alpha = aug(torch.from_numpy(rgb.transpose(0, 3, 1, 2).copy()).to(DEV), torch.from_numpy(depth).to(DEV), 25, list(range(n)))
        rainy, alpha = rainy.cpu().numpy(), alpha.cpu().numpy().reshape(n, KH, KW)
    finally:
        aug.close()
    for i in range(n):
        got = _rgb(os.path.join(out, 'rainy_image', '%06d.png' % i))
        assert np.array_equal(rainy[i].transpose(1, 2, 0), got), i
        lab = np.array(Image.open(os.path.join(out, 'lens_alpha', '%06d.png' % i)))
        assert np.array_equal(lab[..., 0], lens.alpha_label(alpha[i])) and (alpha[i] > 0).any(), i
