"""RR_OPT_STREAK_LEAN: the catalogue of hand-made streaks, the expected frame by composition of the frozen oracle's own functions,
and the host build of the renderer with the mode on (tests/hostemu/lean_emu.cpp).  Shared by tests/test_streak_lean_host.py and
tests/test_gpu_streak_lean.py.

The rule (rr_device.h plan_drop, lean = 1), for a rotated (Medium or Small) tile only: flip = x1 > x0 and the tile's corner is
(min(x0, x1), min(y0, y1)).  The oracle knows the reference's rule only, so the expectation is composed from its
pieces: oracle.render.make_drop_tile reads the frame's width W in one comparison for a non-Big drop -- `end.x > W // 2`, the flip --
so a made-up W forces the flip the rule demands (ALWAYS_FLIP / NEVER_FLIP below), and add_drop_to_image takes the corner as an
argument.  Big drops go through the unchanged functions."""
import ctypes
import os

import numpy as np

import helpers as h
from oracle import render as orc

H, W = 64, 96
ALWAYS_FLIP, NEVER_FLIP = -2_000_000, 2_000_000_000     # W // 2 below / above every int32 x

MED, SMALL, BIG = 2.5, 1.5, 5.0                          # image widths: max_width 2 (Medium), 1 (Small), 5 (Big)
# (name, x0, y0, x1, y1, image width, circle of confusion in pixels): top-left pixel coordinates
CATALOGUE = [
    ('right_down_left_half', 20, 6, 28, 20, MED, 0.0),   # the reference leaves it unflipped ('/'): the rules disagree
    ('left_down_right_half', 62, 4, 54, 18, MED, 0.0),   # the reference flips it and starts the tile at the start: they disagree twice
    ('right_up', 8, 60, 15, 47, MED, 0.0),
    ('left_up', 50, 62, 42, 50, MED, 0.0),
    ('right_down_right_half', 70, 6, 79, 21, MED, 0.0),  # ends in the right half: the two rules agree
    ('vertical', 88, 4, 88, 19, MED, 0.0),
    ('horizontal', 30, 26, 45, 26, MED, 0.0),
    ('small_right_down', 4, 24, 9, 35, SMALL, 0.0),
    ('small_left_down', 92, 24, 86, 36, SMALL, 0.0),
    ('big', 30, 34, 36, 47, BIG, 0.0),
    ('big_left_down', 80, 40, 73, 52, BIG, 0.0),
    ('corner_left_of_frame', 3, 40, -5, 53, MED, 0.0),   # starts inside; min x = -5
    ('corner_above_frame', 40, 5, 45, -7, MED, 0.0),     # starts inside; min y = -7
    ('starts_outside_left', -4, 8, 5, 22, MED, 0.0),     # start outside the frame, end inside
    ('starts_outside_right', 99, 28, 91, 41, MED, 0.0),
    ('overlap_a', 58, 30, 69, 46, MED, 0.0),             # two drops of opposite lean over the same pixels
    ('overlap_b', 69, 30, 58, 46, MED, 0.0),
    ('blurred_left_down', 26, 44, 18, 58, MED, 1.0),     # through the defocus blur
    ('blurred_small_right_up', 52, 60, 57, 49, SMALL, 2.0),
]
NAMES = [c[0] for c in CATALOGUE]


def records(tmp):
    """The catalogue as rr_drop records (the product's loader and packer on helpers.streak particles), in catalogue order."""
    parts = []
    for k, (name, x0, y0, x1, y1, iw, coc) in enumerate(CATALOGUE):
        depth = h.depth_for_coc(coc) if coc > 0 else 6.0
        parts.append(h.streak(k, x0, y0, x1, y1, iw, iw, depth, H, W))
    sc = h.Scene(tmp, H, W, 0, frames=[dict(id=0, t=2000, d=0, drops=parts)])
    rec = sc.product_drops(0)
    assert len(rec) == len(CATALOGUE), 'the frame filter dropped a catalogue entry'
    for r, (name, x0, y0, x1, y1, iw, _) in zip(rec, CATALOGUE):
        assert (int(r['x0']), int(r['y0']), int(r['x1']), int(r['y1'])) == (x0, y0, x1, y1), name
        assert int(r['type']) == (0 if iw == BIG else 1 if iw == MED else 2), name
    return rec


def wanted_flip(r):
    return int(r['x1']) > int(r['x0'])


def tile_covariance(alpha):
    """x-y covariance of a tile's mass (image axes: y grows downward): positive for a tile whose x grows with y."""
    ys, xs = np.mgrid[:alpha.shape[0], :alpha.shape[1]]
    m = alpha.sum()
    return float(((xs - (alpha * xs).sum() / m) * (ys - (alpha * ys).sum() / m) * alpha).sum() / m)


def oracle_lean(scene, bg, env_xyY, recs, faithful=True):
    """oracle.render.render_drop_records with the lean rule, by composition (module docstring)."""
    textures, _ = scene.oracle_db()
    fh, fw = bg.shape[:2]
    rainy_bg = bg.copy()
    rainy_mask = np.zeros((fh, fw), np.float64)
    fc = orc.FrameConsts(env_xyY, scene.omega)
    status = np.zeros(len(recs), np.int32)
    for i, r in enumerate(recs):
        drop = orc.Streak()
        drop.pid = i
        drop.world_position_start = np.array(r['wps'], np.float64)
        drop.world_position_end = np.array(r['wpe'], np.float64)
        drop.image_position_start = np.array([int(r['x0']), int(r['y0'])])
        drop.image_position_end = np.array([int(r['x1']), int(r['y1'])])
        drop.image_diameter_start, drop.image_diameter_end = float(r['iw1']), float(r['iw2'])
        drop.max_width, drop.length = int(r['max_width']), int(r['length'])
        drop.drop_type = orc.DropType(int(r['type']))
        rot = (float(r['rot_cos']), float(r['rot_sin']))
        if drop.drop_type == orc.DropType.Big:
            tile, minC = orc.make_drop_tile(drop, textures[int(r['tex_index'])], 0.0, fw, fh, rot=rot)
        else:
            tile, _ = orc.make_drop_tile(drop, textures[int(r['tex_index'])], 0.0, ALWAYS_FLIP if wanted_flip(r) else NEVER_FLIP, fh, rot=rot)
            minC = np.array([min(int(r['x0']), int(r['x1'])), min(int(r['y0']), int(r['y1']))])
        pts = orc.compute_fov_plane_points(drop.world_position_start, drop.world_position_end, orc.RADIUS, orc.FOV_DEG, orc.N_FOV, env_xyY.shape)
        try:
            orc.add_drop_to_image(env_xyY, scene.omega, fc, pts, minC, bg.shape, rainy_bg, rainy_mask, tile, drop, scene.ocam, 1.0, faithful,
                                  None, None)
        except IndexError as e:
            status[i] = e.args[0] if e.args and isinstance(e.args[0], int) else orc.ST_FOV_FAIL
    return dict(rainy_bg=rainy_bg, mask=rainy_mask, mask_i32=orc.quantise_mask(rainy_mask), image_u8=orc.quantise_image(rainy_bg, bg), status=status)


# ---- the host build with the mode as a run-time switch --------------------------------------------------------------
_lib = None


def lean_emu():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(h.ROOT, 'tests', 'hostemu', 'libleanemu.so'))
    return _lib


class _Lean:
    """helpers.emu_render / emu_plan run on libleanemu.so with the mode `lean` while this is entered."""

    def __init__(self, lean):
        self.lean = int(lean)

    def __enter__(self):
        self.old = h._emu
        h._emu = lean_emu()
        h._emu.emu_set_streak_lean(self.lean)

    def __exit__(self, *exc):
        h._emu.emu_set_streak_lean(0)
        h._emu = self.old


def emu_render(scene, bg, env_xyY, recs, lean):
    with _Lean(lean):
        return h.emu_render(scene, bg, bg, env_xyY, recs)


def emu_plan(scene, recs, lean):
    with _Lean(lean):
        return h.emu_plan(scene, recs)


def check(out, ref, tag):
    """The repository's bar: statuses equal, mask float64 and int32 bit-exact, image within 1 LSB."""
    assert np.array_equal(out['status'], ref['status']), (tag, out['status'], ref['status'])
    assert np.array_equal(out['mask'], ref['mask']), '%s: mask (f64) differs at %d pixels' % (tag, int((out['mask'] != ref['mask']).sum()))
    assert np.array_equal(out['mask_i32'], ref['mask_i32']), '%s: mask (i32) differs' % tag
    d = int(np.abs(out['image_u8'].astype(int) - ref['image_u8'].astype(int)).max())
    assert d <= 1, '%s: image differs by %d LSB' % (tag, d)
