"""GPU tier of the rain layer as a file (rr_pipeline_set_layer_png, k_rain_layer<2>, k_png_layer, k_pngz_*<3 / 4>).

The yardstick is exact: a frame's file bytes are tools/layer_png.py encode() of the float32 layer the SAME batch returned through
rr_pipeline_set_layer on the same slot, and the scanlines are numpy's Sub filter of that.

Shapes (the smallest at which it can go wrong): 61 x 47 (a partial 32-wide tile, partial 16-row quadrants), 40 x 1, 64 x 200 (two 32 KB
deflate blocks, the last one short); every batch is n = 3: all drops, every second drop and no drops (a file that is all zero), and the
second frame's buffer is NULL wherever a test says so.
  1. files == encode(float layer); layer bits, image, mask, statuses == the runs armed with the float layer only and with nothing; the
     file armed alone; the float64 compositor;
  2. RR_OPT_PNG_DEFLATE: zlib inflates the stream to the scanlines; rr_io_write_frames_text's file reads back equal;
  3. three armed slots in flight, one armed among three, disarming;
  4. lens, lens label and layer file together (four streams); the layer is that of the streaks alone;
  5. every refusal, each followed by a good call; rr_render_frames_device;
  6. the re-submit after an arena regrowth;
  7. recomposition on segment_dim within 2 codes, no pixel excluded;
  8. main.py --device_particles --rain_layer against RainAugment(return_layer=True); the XML route; RAIN_NATIVE_IO=0."""
import ctypes
import importlib
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import helpers as h
import lens_cases as lc
import rain_layer as rl
import compositor_cases as cc
import test_gpu_compositor_cases as tcc
import test_gpu_edge_cases as edge
import test_gpu_prepass as tp
from test_gpu_augment import DEV, streaks_db          # noqa: F401  (streaks_db: a fixture)
from test_gpu_driver import _make_dataset
from test_gpu_pipeline_async import _defocused_frames

pytestmark = pytest.mark.gpu

hb = h.hb
lens = lc.lens
lp = importlib.import_module('rain-rendering_amd.tools.layer_png')
imgops = importlib.import_module('rain-rendering_amd.common.imgops')
augment = importlib.import_module('rain-rendering_amd.augment')
main_mod = importlib.import_module('rain-rendering_amd.main')
RR_E_ARG, RR_E_STATE = -1, -4
SHAPES = {'odd': (61, 47, 80), 'column': (40, 1, 400), 'blocks': (64, 200, 150)}
KEYS = ('image_u8', 'mask', 'mask_i32', 'status')


class World:
    """One shape: scene, context, the batch of three frames, and the four baseline runs (made once, never changed)."""

    def __init__(self, tmp, name):
        self.name = name
        self.H, self.W, n_drops = SHAPES[name]
        H, W = self.H, self.W
        self.sc = sc = h.Scene(tmp, H, max(W, 47), n_drops, n_frames=1, seed0=77)
        bg, env = sc.frame_inputs(0)
        if W == 1:                                                    # the product's own filter for a one-pixel-wide frame
            table = list(sc.db.streaks_simulator.values())[0].table
            np.random.seed(0)
            drops = hb.pack_drops(table, hb.filter_streaks(table, W, H), sc.db, 0.0, 0.0)
            bg = np.ascontiguousarray(bg[:, :1])
        else:
            drops = sc.product_drops(0)
        assert len(drops) >= 4
        self.rh = rh = hb.RainHip(0)
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        rh.set_colormap(imgops.viridis_lut())
        self.tables = [drops, drops[::2], np.zeros(0, hb.DROP_DTYPE)]
        self.frames = [dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=t) for t in self.tables]
        self.bg = bg
        self.row = H * (1 + 4 * W)
        self.nothing = self.run(0)
        self.float_only = self.run(0, lay=True)
        self.both = self.run(0, lay=True, png=(True, True, True))
        for r in (self.nothing, self.float_only, self.both):
            for o in r['outs']:
                for a in o.values():
                    a.setflags(write=False)

    def outs(self, frames, composite=False, files=False):
        H, W = self.H, self.W
        o = [dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W)), mask_i32=np.zeros((H, W), np.int32),
                  status=np.zeros(len(f['drops']), np.int32)) for f in frames]
        for d in o:
            if composite:
                d['rainy_bg'] = np.zeros((H, W, 3))
            if files:
                d['rainy_png'], d['mask_png'] = np.full(self.row, 9, np.uint8), np.full(self.row, 9, np.uint8)
        return o

    def arm(self, slot, n, lay, png):
        """-> (float buffers or None, file buffers (None entries: NULL pointers) or None); sentinels everywhere."""
        rh, H, W = self.rh, self.H, self.W
        fl = pg = None
        if lay:
            fl = [dict(layer=np.full((H, W, 4), -7.0, np.float32), shift=np.full(1, -7.0)) for _ in range(n)]
            rh.pipeline_set_layer(slot, fl)
        if png is not None:
            pg = [np.full(self.row, 9, np.uint8) if png[k] else None for k in range(n)]
            rh.pipeline_set_layer_png(slot, pg, H, W)
        return fl, pg

    def submit(self, slot, frames, o):
        self.rh.pipeline_submit(slot, frames, o)

    def wait(self, slot, frames, o):
        while not self.rh.pipeline_wait(slot):                        # (RR_E_ARENA: the re-submit applies the armed state once more)
            self.submit(slot, frames, o)

    def disarm(self, slot):
        self.rh.pipeline_set_layer(slot, None)
        self.rh.pipeline_set_layer_png(slot, None)

    def run(self, slot, lay=False, png=None, frames=None, composite=False, files=False):
        frames = self.frames if frames is None else frames
        o = self.outs(frames, composite, files)
        fl, pg = self.arm(slot, len(frames), lay, png)
        try:
            self.submit(slot, frames, o)
            self.wait(slot, frames, o)
        finally:
            self.disarm(slot)
        return dict(outs=o, lay=fl, png=pg)


@pytest.fixture(scope='module')
def worlds(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(tmp_path_factory.mktemp('lpng_' + name), name)
        return made[name]
    yield get
    for w in made.values():
        w.rh.close()


def _rows_of(layer):
    """The scanlines of a float32 layer [H, W, 4]: the statement, then numpy's Sub filter."""
    return lp.sub_filter(lp.encode(layer)).ravel()


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), '%s: %s differs' % (what, k)


def _check_files(w, res, frames_with_file, what):
    for f in range(3):
        lay = w.both['lay'][f]['layer']
        if f in frames_with_file:
            got, want = res['png'][f], _rows_of(lay)
            diff = np.flatnonzero(got != want)
            print('%s %s frame %d: %d of %d scanline bytes differ' % (w.name, what, f, len(diff), want.size), diff[:6].tolist())
            assert np.array_equal(got, want), (what, f)
        else:
            assert res['png'][f] is None


# ---- 1. the files are the statement of the float layer ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SHAPES))
def test_file_bytes_equal_the_statement_of_the_float_layer(worlds, name):
    w = worlds(name)
    _check_files(w, w.both, (0, 1, 2), 'both armed')
    for f in range(3):
        lay = w.both['lay'][f]
        assert np.array_equal(lay['layer'].view(np.uint32), w.float_only['lay'][f]['layer'].view(np.uint32)), f      # the layer's bits
        assert lay['shift'][0] == w.float_only['lay'][f]['shift'][0] and lay['shift'][0] != -7.0
        _same(w.both['outs'][f], w.float_only['outs'][f], 'both vs float only, frame %d' % f)
        _same(w.both['outs'][f], w.nothing['outs'][f], 'both vs nothing, frame %d' % f)
    rgba = lp.encode(w.both['lay'][0]['layer'])
    assert rgba[..., 3].max() > 0 and rgba[..., :3].max() > 0 and w.nothing['outs'][0]['mask'].max() > 0      # streaks are shown
    empty = w.both['png'][2].reshape(w.H, 1 + 4 * w.W)                   # the frame without drops: a file that is all zero
    assert (empty[:, 0] == 1).all() and not empty[:, 1:].any()
    assert (w.both['lay'][2]['layer'][..., 3] == 1).all()


@pytest.mark.parametrize('name', list(SHAPES))
def test_file_armed_alone_and_a_null_pointer(worlds, name):
    w = worlds(name)
    alone = w.run(0, lay=False, png=(True, False, True))
    _check_files(w, alone, (0, 2), 'file alone')
    for f in range(3):
        _same(alone['outs'][f], w.nothing['outs'][f], 'file alone vs nothing, frame %d' % f)
    mixed = w.run(1, lay=True, png=(False, True, False))                 # another slot; the float layer of every frame, one file
    _check_files(w, mixed, (1,), 'one file')
    for f in range(3):
        assert np.array_equal(mixed['lay'][f]['layer'].view(np.uint32), w.both['lay'][f]['layer'].view(np.uint32)), f


@pytest.mark.parametrize('name', ['odd', 'column'])
def test_float64_compositor_gives_the_same_bytes(worlds, name):
    """The layer's colour constants follow RR_OPT_FOV_F32, whose default depends on the compositor: with the float64
    constants everywhere the layer's bits, and so the file's bytes, are the same under every compositor."""
    w = worlds(name)
    rh = w.rh
    every = (True, True, True)
    rh.set_option(hb.RR_OPT_FOV_F32, 0)
    try:
        base = w.run(0, lay=True, png=every)
        comp = w.run(0, lay=True, png=every, composite=True)
        rh.set_option(hb.RR_OPT_COMPOSITE_F64, 1)
        try:
            opt = w.run(0, lay=True, png=every)
            alone = w.run(0, png=every)
        finally:
            rh.set_option(hb.RR_OPT_COMPOSITE_F64, 0)
    finally:
        rh.set_option(hb.RR_OPT_FOV_F32, 2)
    for f in range(3):
        assert np.array_equal(base['png'][f], _rows_of(base['lay'][f]['layer'])), f
        for what, res in (('composite asked for', comp), ('RR_OPT_COMPOSITE_F64', opt)):
            assert np.array_equal(res['lay'][f]['layer'].view(np.uint32), base['lay'][f]['layer'].view(np.uint32)), (what, f)
            assert np.array_equal(res['png'][f], base['png'][f]), (what, f)
        assert np.array_equal(alone['png'][f], base['png'][f]), f
        assert comp['outs'][f]['rainy_bg'].max() > 0
    # and under the defaults the float64 composite's file is the statement of its own batch's layer
    own = w.run(0, lay=True, png=every, composite=True)
    for f in range(3):
        assert np.array_equal(own['png'][f], _rows_of(own['lay'][f]['layer'])), f


# ---- 2. entropy-coded on the device ----------------------------------------------------------------------------------------------
def _payload(buf, n_bytes):
    """The scanlines a downloaded buffer stands for: an RRZ1 stream inflated by zlib, or the scanlines themselves."""
    if buf[:4].tobytes() != b'RRZ1':
        return buf, False
    hd = np.frombuffer(buf[:16].tobytes(), np.uint32)
    assert hd[2] == 0 and hd[3] == 0 and 16 + int(hd[1]) <= n_bytes
    return np.frombuffer(zlib.decompress(buf[16:16 + int(hd[1])].tobytes()), np.uint8), True


@pytest.mark.parametrize('name', ['blocks', 'odd', 'column'])
def test_deflate_on_the_device(worlds, name, tmp_path):
    w = worlds(name)
    rh = w.rh
    rh.set_option(hb.RR_OPT_PNG_DEFLATE, 1)
    try:
        plain = w.run(0, files=True)
        got = w.run(0, lay=True, png=(True, False, True), files=True)
    finally:
        rh.set_option(hb.RR_OPT_PNG_DEFLATE, 0)
    coded = []
    for f in (0, 2):
        rows, was_coded = _payload(got['png'][f], w.row)
        coded.append(was_coded)
        assert np.array_equal(rows, _rows_of(w.both['lay'][f]['layer'])), f
    print('%s: layer streams entropy-coded: %s' % (name, coded))
    assert all(coded) or name == 'column'                                # (a 5-byte row may not pay for its header)
    assert got['png'][1] is None
    for f in range(3):                                                   # the other two streams are what they are without the layer
        for k in ('rainy_png', 'mask_png'):
            assert np.array_equal(got['outs'][f][k], plain['outs'][f][k]), (f, k)
        assert _payload(plain['outs'][f]['rainy_png'], w.row)[0][0] == 1
    # the file: written from the stream as it is, read back
    stride = (w.row + 15) // 16 * 16
    block = np.zeros((3, stride), np.uint8)
    for f in (0, 2):
        block[f, :w.row] = got['png'][f]
    paths = [str(tmp_path / ('l%d.png' % f)) for f in range(3)]
    texts = [repr(float(got['lay'][f]['shift'][0])) for f in range(3)]
    paths[1] = None
    assert not hb.io_write_frames_text(paths, block, w.W, w.H, lp.SHIFT_KEYWORD, texts).any()
    for f in (0, 2):
        with Image.open(paths[f]) as im:
            assert np.array_equal(np.array(im), lp.encode(w.both['lay'][f]['layer'])) and im.text == {lp.SHIFT_KEYWORD: texts[f]}
        layer, shift = imgops.read_rain_layer(paths[f])
        assert shift == w.both['lay'][f]['shift'][0]
        src = w.both['lay'][f]['layer'].astype(np.float64)
        inside = bool((src[..., :3] >= 0).all() and (src[..., :3] <= 1 - src[..., 3:]).all() and (src[..., 3] >= 0).all() and (src[..., 3] <= 1).all())
        print('%s frame %d: max |decoded - float layer| %.6g (bound %.6g, condition %s)' % (name, f, np.abs(layer - src).max(), lp.BOUND, inside))
        assert not inside or np.abs(layer - src).max() <= lp.BOUND


# ---- 3. slots --------------------------------------------------------------------------------------------------------------------
def test_three_armed_slots_in_flight_then_one_among_three_then_none(worlds):
    w = worlds('odd')
    rh = w.rh
    for armed in ((0, 1, 2), (1,), ()):
        o = [w.outs(w.frames[s:s + 1]) for s in range(3)]
        bufs = [w.arm(s, 1, True, (True,)) if s in armed else (None, [np.full(w.row, 9, np.uint8)]) for s in range(3)]
        try:
            for s in range(3):
                w.submit(s, w.frames[s:s + 1], o[s])                    # frame s on slot s, all in flight together
            for s in range(3):
                w.wait(s, w.frames[s:s + 1], o[s])
        finally:
            for s in range(3):
                w.disarm(s)
        for s in range(3):
            _same(o[s][0], w.nothing['outs'][s], 'armed %s, slot %d' % (armed, s))
            if s in armed:
                assert np.array_equal(bufs[s][1][0], _rows_of(w.both['lay'][s]['layer'])), (armed, s)
                assert np.array_equal(bufs[s][0][0]['layer'].view(np.uint32), w.both['lay'][s]['layer'].view(np.uint32)), (armed, s)
            else:
                assert (bufs[s][1][0] == 9).all()                        # never armed, or disarmed: nothing is written
    # disarming one of the two leaves the other
    fl, pg = w.arm(0, 3, True, (True, True, True))
    rh.pipeline_set_layer_png(0, None)
    o = w.outs(w.frames)
    try:
        w.submit(0, w.frames, o)
        w.wait(0, w.frames, o)
    finally:
        w.disarm(0)
    assert all((p == 9).all() for p in pg)
    assert all(np.array_equal(fl[f]['layer'].view(np.uint32), w.both['lay'][f]['layer'].view(np.uint32)) for f in range(3))
    # the synchronous calls run on slot 0
    pg = [np.full(w.row, 9, np.uint8) for _ in range(3)]
    rh.pipeline_set_layer_png(0, pg, w.H, w.W)
    try:
        sync = rh.render_frames(w.frames, want_composite=False)
    finally:
        rh.pipeline_set_layer_png(0, None)
    for f in range(3):
        assert np.array_equal(pg[f], _rows_of(w.both['lay'][f]['layer'])) and np.array_equal(sync[f]['image_u8'], w.nothing['outs'][f]['image_u8'])


# ---- 4. lens, lens label and layer file: four streams --------------------------------------------------------------------------
@pytest.mark.parametrize('deflate', [0, 1])
def test_lens_label_and_layer_together(worlds, deflate):
    w = worlds('blocks')
    rh, H, W = w.rh, w.H, w.W
    L = lens.LensDrops(H, W, count=8, radius=(2, 10), life_s=(0.2, 0.4), seed=0)
    tabs = [L.table(i) for i in range(3)]
    assert all(len(t) >= 3 for t in tabs)

    def run(with_layer):
        o = w.outs(w.frames, files=True)
        label = [np.full(w.row, 9, np.uint8) for _ in range(3)]
        rh.pipeline_set_lens(0, tabs, L.weights(), H, W, alpha_png=label)
        fl, pg = w.arm(0, 3, with_layer, (True, True, True) if with_layer else None)
        try:
            w.submit(0, w.frames, o)
            w.wait(0, w.frames, o)
        finally:
            w.disarm(0)
            rh.pipeline_set_lens(0, None)
        return o, label, fl, pg

    rh.set_option(hb.RR_OPT_PNG_DEFLATE, deflate)
    try:
        o3, label3, _, _ = run(False)
        o4, label4, fl, pg = run(True)
    finally:
        rh.set_option(hb.RR_OPT_PNG_DEFLATE, 0)
    for f in range(3):
        rows, coded = _payload(pg[f], w.row)
        assert coded == bool(deflate)
        assert np.array_equal(rows, _rows_of(w.both['lay'][f]['layer'])), f      # the streaks alone: the bytes without the lens
        assert np.array_equal(fl[f]['layer'].view(np.uint32), w.both['lay'][f]['layer'].view(np.uint32)), f
        assert np.array_equal(label4[f], label3[f]) and not (label4[f] == 9).all(), f
        for k in KEYS + ('rainy_png', 'mask_png'):
            assert np.array_equal(o4[f][k], o3[f][k]), (f, k)
        assert not np.array_equal(o4[f]['image_u8'], w.nothing['outs'][f]['image_u8'])      # the lens drops are worn
        assert np.array_equal(o4[f]['mask'], w.nothing['outs'][f]['mask'])


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def _arg(bufs, n, H, W):
    ptrs = (ctypes.c_void_p * max(len(bufs), 1))(*[None if a is None else a.ctypes.data for a in bufs])
    b = hb.rr_pipeline_layer_png()
    b.n, b.H, b.W, b.layer_png = n, H, W, ctypes.cast(ptrs, ctypes.c_void_p)
    return b, ptrs


def test_refusals(worlds):
    w = worlds('odd')
    rh, H, W = w.rh, w.H, w.W
    lib, hnd = rh.lib, rh.h
    bufs = [np.full(w.row, 9, np.uint8) for _ in range(3)]

    def err():
        return lib.rr_last_error(hnd).decode()

    def refused(what, slot, n, hh, ww, null=False):
        b, keep = _arg(bufs, n, hh, ww)
        if null:
            b.layer_png = None
        assert lib.rr_pipeline_set_layer_png(hnd, slot, ctypes.byref(b)) == RR_E_ARG, what
        assert err().startswith('rr_pipeline_set_layer_png'), what

    refused('slot -1', -1, 3, H, W)
    refused('slot 3', 3, 3, H, W)
    refused('n = 0', 0, 0, H, W)
    refused('n < 0', 0, -2, H, W)
    refused('H = 0', 0, 3, 0, W)
    refused('W < 0', 0, 3, H, -1)
    refused('a null table', 0, 3, H, W, null=True)
    # nothing changed: slot 0 is still unarmed
    good = w.run(0)
    for f in range(3):
        _same(good['outs'][f], w.nothing['outs'][f], 'after the refused arming calls')
    assert all((b == 9).all() for b in bufs)
    # a slot in flight can be neither armed nor disarmed
    o = w.outs(w.frames)
    w.submit(2, w.frames, o)
    b, keep = _arg(bufs, 3, H, W)
    assert lib.rr_pipeline_set_layer_png(hnd, 2, ctypes.byref(b)) == RR_E_STATE and 'in flight' in err()
    assert lib.rr_pipeline_set_layer_png(hnd, 2, None) == RR_E_STATE
    w.wait(2, w.frames, o)
    for f in range(3):
        _same(o[f], w.nothing['outs'][f], 'slot 2 (never armed)')
    assert all((b == 9).all() for b in bufs)
    # a submit that does not match the armed batch: RR_E_ARG, nothing enqueued
    try:
        for n, hh, ww in ((2, H, W), (3, H + 1, W), (3, H, W + 1)):
            rh.pipeline_set_layer_png(1, bufs[:n], hh, ww) if (hh, ww) == (H, W) else \
                rh.pipeline_set_layer_png(1, [np.full(hh * (1 + 4 * ww), 9, np.uint8) for _ in range(n)], hh, ww)
            o = w.outs(w.frames)
            with pytest.raises(RuntimeError, match=r'\(-1\).*armed with rr_pipeline_set_layer_png'):
                rh.pipeline_submit(1, w.frames, o)
            assert rh.pipeline_wait(1) and not o[0]['image_u8'].any() and all((b == 9).all() for b in bufs)
        rh.pipeline_set_layer_png(1, bufs, H, W)                         # the next good batch is correct
        o = w.outs(w.frames)
        w.submit(1, w.frames, o)
        w.wait(1, w.frames, o)
        for f in range(3):
            assert np.array_equal(bufs[f], _rows_of(w.both['lay'][f]['layer'])), f
            _same(o[f], w.nothing['outs'][f], 'the valid batch behind the refused ones')
        # a batch that renders nothing (the pre-pass alone runs on slot 0)
        consts, _ = tp._setup(rh, H, W, 25)
        rh.pipeline_set_layer_png(0, bufs[:1], H, W)
        bg, depth = tp._scene(H, W, 3)
        with pytest.raises(RuntimeError, match='renders nothing'):
            rh.prepass_frames([dict(bg=bg, depth=depth, fog=consts)])
        # rr_render_frames_device: the file route is the host entry points'
        fin, fout = (hb.rr_frame_in * 1)(), (hb.rr_frame_out * 1)()
        with pytest.raises(RuntimeError, match=r'\(-1\).*rr_pipeline_set_layer_png'):
            rh.render_frames_device(fin, fout, 1)
    finally:
        for s in range(3):
            rh.pipeline_set_layer_png(s, None)
    again = w.run(0, lay=True, png=(True, True, True))
    _check_files(w, again, (0, 1, 2), 'after the refusals')
    with pytest.raises(ValueError):
        rh.pipeline_set_layer_png(0, [np.zeros(5, np.uint8)], H, W)


# ---- 6. arena regrowth -----------------------------------------------------------------------------------------------------------
def test_resubmit_after_arena_regrowth(tmp_path, built):
    sc = h.Scene(tmp_path, edge.H, edge.W, 0, frames=_defocused_frames(420))
    bg, env = sc.frame_inputs(0)
    drops = sc.product_drops(0)
    fr = dict(bg=bg, rainy_bg=bg, env_xyY=env, omega=sc.omega, drops=drops)
    H, W = edge.H, edge.W
    rh = hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)

        def out():
            return dict(image_u8=np.zeros((H, W, 3), np.uint8), mask=np.zeros((H, W)), mask_i32=np.zeros((H, W), np.int32),
                        status=np.zeros(len(drops), np.int32))
        armed, plain = out(), out()
        png = np.full(H * (1 + 4 * W), 9, np.uint8)
        lay = dict(layer=np.full((H, W, 4), -7.0, np.float32), shift=np.full(1, -7.0))
        rh.pipeline_set_layer_png(0, [png], H, W)
        rh.pipeline_set_layer(0, [lay])
        rh.pipeline_submit(0, [fr], [armed])
        assert rh.pipeline_wait(0) is False                           # the first wait reports the regrowth
        rh.pipeline_submit(0, [fr], [armed])                          # the armed state is still on the slot
        assert rh.pipeline_wait(0) is True
        rh.pipeline_set_layer_png(0, None)
        rh.pipeline_set_layer(0, None)
        rh.pipeline_submit(0, [fr], [plain])
        assert rh.pipeline_wait(0) is True
        assert np.array_equal(png, _rows_of(lay['layer'])) and lp.encode(lay['layer'])[..., 3].max() > 0
        for k in KEYS:
            assert np.array_equal(armed[k], plain[k]), k
    finally:
        rh.close()


# ---- 7. recomposition ------------------------------------------------------------------------------------------------------------
def test_the_file_over_the_background_is_the_rainy_image(built, tmp_path_factory):
    """segment_dim, for which rain_layer.reference() asserts on the reference alone that no blend clamped: the composite is
    T rainy_bg + L.  |rainy_rgb - trunc(clip01(T' rainy_bg + L' - shift) 255)| <= 2 everywhere: the layer contract's 1 LSB plus the
    1/255 of the file's quantisation.  Measured on an MI355X: max 1 code."""
    c = rl.segment_dim(tmp_path_factory.mktemp('sd'), cc.Templates(tmp_path_factory.mktemp('tpl')))
    rl.reference(c)                                                   # (asserts the condition)
    rh = tcc._ctx(c)
    try:
        png = np.full(c.H * (1 + 4 * c.W), 9, np.uint8)
        lay = dict(layer=None, shift=np.full(1, -7.0))                # the driver's arming: the shift alone, and the file
        rh.pipeline_set_layer_png(0, [png], c.H, c.W)
        rh.pipeline_set_layer(0, [lay])
        out = rh.render_frames([c.frame()], want_composite=False)[0]
    finally:
        rh.pipeline_set_layer_png(0, None)
        rh.pipeline_set_layer(0, None)
        rh.close()
    rows = png.reshape(c.H, 1 + 4 * c.W)
    assert (rows[:, 0] == 1).all()
    rgba = (np.cumsum(rows[:, 1:].reshape(c.H, c.W, 4).astype(np.int64), axis=1) % 256).astype(np.uint8)      # the Sub filter undone
    lb, lg, lr, t = lp.decode(rgba)
    L = np.stack([lb, lg, lr], axis=-1)
    v = np.clip(t[..., None] * c.bg + L - lay['shift'][0], 0.0, 1.0)
    rgb = (v * 255.0).astype(np.uint8)[..., ::-1]                     # B G R -> R G B
    d = np.abs(rgb.astype(int) - out['image_u8'].astype(int))
    print('segment_dim: shift %.6g, measured max |d| %d codes, %d px differ, alpha codes up to %d' % (
        lay['shift'][0], d.max(), (d > 0).any(axis=2).sum(), rgba[..., 3].max()))
    assert d.max() <= 2, cc.where(c, (d > 2).any(axis=2), cc.GEOM32)
    assert rgba[..., 3].max() > 0 and (out['mask'] > 0).any()


# ---- 8. the driver ---------------------------------------------------------------------------------------------------------------
def _drive(tmp, src, streaks, out_name, extra, monkeypatch, native=True, rate='5'):
    monkeypatch.setenv('RAIN_NATIVE_IO', '1' if native else '0')
    monkeypatch.setenv('RAIN_BATCH', '2')                             # two batches, a ragged last one
    gen = main_mod.main(['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', streaks, '-i', rate,
                         '--output', os.path.join(tmp, out_name), '--noverbose'] + list(extra))
    assert len(gen.stats) == 3
    return gen, os.path.join(tmp, out_name, 'kitti', 'data_object', 'training', 'rain', rate + 'mm')


KH, KW = 375, 1242                                         # KITTI's frames: the device's particle generator renders the sensor's size


def test_driver_device_particles_equals_rain_augment(built, tmp_path_factory, streaks_db):
    tmp = str(tmp_path_factory.mktemp('layerdriver'))
    src = os.path.join(tmp, 'source')
    h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), 3, KH, KW, depth_m=None)
    with pytest.MonkeyPatch.context() as mp:
        gen, out = _drive(tmp, src, streaks_db, 'layer', ['--device_particles', '--rain_layer'], mp, rate='25')
        assert gen.timing[0].get('route') == 'native'
        _, out_plain = _drive(tmp, src, streaks_db, 'plain', ['--device_particles'], mp, rate='25')
    assert not os.path.exists(os.path.join(out_plain, 'rain_layer'))
    n = 3
    img_dir = os.path.join(src, 'kitti', 'data_object', 'training', 'image_2')
    rgb = np.stack([np.array(Image.open(os.path.join(img_dir, '%06d.png' % i)).convert('RGB')) for i in range(n)])
    depth = np.stack([np.array(Image.open(os.path.join(img_dir, 'depth', '%06d.png' % i))).astype(np.float32) / 256. for i in range(n)])
    aug = augment.RainAugment('kitti', streaks_db=streaks_db, sequence='data_object/training', return_layer=True)
    try:
        rainy, mask, layer = aug(torch.from_numpy(rgb.transpose(0, 3, 1, 2).copy()).to(DEV), torch.from_numpy(depth).to(DEV), 25, list(range(n)))
        planes, shift, rainy = layer.planes.cpu().numpy(), layer.shift.cpu().numpy(), rainy.cpu().numpy()
        background = layer.background.cpu().numpy().astype(np.float64)
    finally:
        aug.close()
    for i in range(n):
        for kind in ('rainy_image', 'rain_mask'):                        # byte-identical to the run without the flag
            a = open(os.path.join(out, kind, '%06d.png' % i), 'rb').read()
            assert a == open(os.path.join(out_plain, kind, '%06d.png' % i), 'rb').read() and len(a) > 300, (kind, i)
        p = os.path.join(out, 'rain_layer', '%06d.png' % i)
        want = lp.encode(np.ascontiguousarray(planes[i][[2, 1, 0, 3]].transpose(1, 2, 0)))      # planes R G B T -> (L_B, L_G, L_R, T)
        with Image.open(p) as im:
            got, text = np.array(im), dict(im.text)
        print('frame %d: %d file bytes differ from encode(RainAugment layer); chunk %r, augment shift %r' % (
            i, int((got != want).sum()), text, float(shift[i])))
        assert np.array_equal(got, want), i
        assert text == {lp.SHIFT_KEYWORD: repr(float(shift[i]))}, i
        assert want[..., 3].max() > 0
        # the reader; and, reported only, the file over the rain-free target: the synthetic map is bright, its drops are outside
        # the condition kg <= te (L > 1 - T: the colour saturates at 255), so the 2 codes of segment_dim are not promised here
        lay, sh = imgops.read_rain_layer(p)
        assert sh == float(shift[i]) and lay.shape == (KH, KW, 4)
        src = planes[i].astype(np.float64)
        outside = (src[:3] > 1.0 - src[3:]).any(axis=0)
        bgd = background[i].transpose(1, 2, 0)[..., ::-1]             # planar R G B -> [H, W, 3] B G R
        v = np.clip(lay[..., 3:4] * bgd + lay[..., :3] - sh, 0.0, 1.0)
        d = np.abs((v * 255.0).astype(np.uint8)[..., ::-1].astype(int) - rainy[i].transpose(1, 2, 0).astype(int)).max(axis=2)
        print('frame %d: %d px outside the condition; the file over the background vs rainy: max %d codes there, %d inside it' % (
            i, int(outside.sum()), d[outside].max() if outside.any() else 0, d[~outside].max()))


def test_driver_xml_route_and_general_route(tmp_path, built, monkeypatch):
    """No --device_particles (the particle file's drops, packed by the host); and RAIN_NATIVE_IO=0, the general route, writes the same
    three files per frame as the native one.  --lens_drops --lens_alpha beside it: all four files, the layer that of the streaks alone."""
    tmp = str(tmp_path)
    src, xml = _make_dataset(tmp)
    streaks = os.path.join(tmp, 'rainstreakdb')
    gen, out_n = _drive(tmp, src, streaks, 'native', ['--rain_layer'], monkeypatch)
    assert gen.timing[0].get('route') == 'native'
    gen_g, out_g = _drive(tmp, src, streaks, 'general', ['--rain_layer'], monkeypatch, native=False)
    assert gen_g.timing[0].get('route') != 'native'
    _, out_p = _drive(tmp, src, streaks, 'plain', [], monkeypatch)
    _, out_l = _drive(tmp, src, streaks, 'lens', ['--rain_layer', '--lens_drops', '8,1', '--lens_alpha'], monkeypatch)
    for i in range(3):
        for kind in ('rainy_image', 'rain_mask', 'rain_layer'):
            a = open(os.path.join(out_n, kind, '%06d.png' % i), 'rb').read()
            assert a == open(os.path.join(out_g, kind, '%06d.png' % i), 'rb').read() and len(a) > 200, (kind, i)
            if kind != 'rain_layer':
                assert a == open(os.path.join(out_p, kind, '%06d.png' % i), 'rb').read(), (kind, i)
        a = open(os.path.join(out_n, 'rain_layer', '%06d.png' % i), 'rb').read()
        assert a == open(os.path.join(out_l, 'rain_layer', '%06d.png' % i), 'rb').read(), i
        assert os.path.exists(os.path.join(out_l, 'lens_alpha', '%06d.png' % i))
        lay, sh = imgops.read_rain_layer(os.path.join(out_n, 'rain_layer', '%06d.png' % i))
        assert sh is not None and lay[..., 3].min() < 1
