"""Shared fixtures for the test tiers: synthetic scene construction in the reference's
on-disk formats, loading through BOTH the product loaders and the oracle loaders, and the
ctypes view of the host-emulation library (tests/hostemu)."""
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pkg = importlib.import_module("rain-rendering_amd")
hb = importlib.import_module("rain-rendering_amd.hip_backend")
synthetic = importlib.import_module("rain-rendering_amd.synthetic")
bw = importlib.import_module("rain-rendering_amd.common.bad_weather")
my_utils = importlib.import_module("rain-rendering_amd.common.my_utils")
solid_angle = importlib.import_module("rain-rendering_amd.common.solid_angle")

from oracle import render as orc  # noqa: E402

scenes = importlib.import_module("rain-rendering_amd.scenes")
KITTI, CITYSCAPES, NUSCENES = scenes.KITTI, scenes.CITYSCAPES, scenes.NUSCENES


class Scene(scenes.Scene):
    """The product-side synthetic sequence (rain-rendering_amd/scenes.py) plus the ORACLE loaders of the
    same files, so a test can feed identical inputs to both."""

    def oracle_streaks(self, i):
        sim = orc.load_streaks_from_xml(self.xml, self.render_scale, [self.W, self.H])
        frames = list(sim.values())
        fr = frames[i % len(frames)]
        return list(orc.streak_filter(fr.streaks, self.W, self.H).values())

    def oracle_db(self):
        return orc.load_streak_database(self.tex_dir, self.norm)


# ---------------------------------------------------------------------------
# host emulation of the kernel arithmetic (tests/hostemu)
# ---------------------------------------------------------------------------
_emu = None


def build_hostemu():
    """The path of libhostemu.so, rebuilt where it is older than its sources: build()'s own recipe and dependency list."""
    return importlib.import_module('__graft_entry__').build_emu('hostemu')


def hostemu():
    global _emu
    if _emu is None:
        _emu = ctypes.CDLL(build_hostemu())
    return _emu


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_render(scene, bg, rainy_bg, env_xyY, drops, opacity=1.0, strategy=0, depth=None):
    emu = hostemu()
    texels, hs, ws, offs = hb.pack_streak_db(scene.db.streaks_light)
    H, W = bg.shape[:2]
    n = len(drops)
    out = dict(image_u8=np.zeros((H, W, 3), np.uint8), rainy_bg=np.zeros((H, W, 3)), mask=np.zeros((H, W)),
               mask_i32=np.zeros((H, W), np.int32), status=np.zeros(max(n, 1), np.int32), K=np.zeros((max(n, 1), 3)))
    drops = np.ascontiguousarray(drops)
    if depth is not None:
        depth = np.ascontiguousarray(depth, np.float32 if np.asarray(depth).dtype == np.float32 else np.float64)
        assert depth.shape == (H, W)
    emu.emu_render_frame_depth(H, W, scene.He, scene.We, _p(bg), _p(rainy_bg), _p(env_xyY), _p(scene.omega), _p(drops), n,
                               ctypes.byref(scene.cam), ctypes.c_double(opacity), _p(texels), _p(hs), _p(ws), _p(offs),
                               _p(out['image_u8']), _p(out['rainy_bg']), _p(out['mask']), _p(out['mask_i32']), _p(out['status']),
                               _p(out['K']), int(strategy), _p(depth) if depth is not None else None,
                               1 if depth is not None and depth.dtype == np.float64 else 0)
    out['status'] = out['status'][:n]
    return out


# the kernels' per-drop plan (rr_device.h DropPlan), as emu_plan writes it
PLAN_DTYPE = np.dtype([(k, '<i4') for k in ('status kind tex flip tw th shift pw ph r1 r2 vis_x0 vis_y0 vis_w vis_h crop_x crop_y ew bw0 nW nH '
                                            'rs_mode isx isy eh epitch epad').split()] + [('pad_', '<i4'), ('a0_off', '<i8'), ('a1_off', '<i8'),
                      ('sig1', '<f8'), ('sig2', '<f8'), ('tau_one', '<f8'), ('g', '<f8'), ('mi', '<f8', (9,)), ('ma', '<f8', (6,)),
                      ('scale_x', '<f8'), ('scale_y', '<f8'), ('inv_sx', '<f8'), ('inv_sy', '<f8')])


def emu_plan(scene, drops, opacity=1.0):
    """The plans k_plan makes for `drops` on the scene's frame (host build): (plans, sizes).  sizes[i] == 0 for a drop that
    renders nothing (a status, no FOV polygon, or a footprint outside the frame) -- the drops the work lists leave out."""
    emu = hostemu()
    assert emu.emu_sizeof_plan() == PLAN_DTYPE.itemsize
    texels, hs, ws, offs = hb.pack_streak_db(scene.db.streaks_light)
    drops = np.ascontiguousarray(drops)
    n = len(drops)
    plans = np.zeros(n, PLAN_DTYPE)
    poly, npts, sizes = np.zeros(max(n, 1) * 72, np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64)
    emu.emu_plan(_p(drops), n, ctypes.byref(scene.cam), scene.H, scene.W, scene.He, scene.We, _p(hs), _p(ws), ctypes.c_double(opacity),
                 _p(plans), _p(poly), _p(npts), _p(sizes))
    return plans, sizes[:n]


# ---------------------------------------------------------------------------
# hand-built streaks
# ---------------------------------------------------------------------------
SENSOR_PX = 4.65e-6                     # the circle of confusion is in these pixels whatever the camera (bad_weather.py:469)


def depth_for_coc(c, cam=KITTI, focus_plane=6.0):
    """The depth (m, in front of the focus plane) whose circle of confusion is c pixels: compute_circle
    c = (6 - o) f^2 / (o (6 - f) N px) solved for o."""
    f, N = cam['focal_mm'] / 1000., cam['f_number']
    return focus_plane * f * f / (c * SENSOR_PX * (focus_plane - f) * N + f * f)


def streak(pid, x0, y0, x1, y1, iw1, iw2, depth, H, W, cam=KITTI):
    """One particle of the XML (synthetic.write_particles_xml) whose streak runs from image (x0, y0) to (x1, y1) in TOP-LEFT
    pixel coordinates at `depth` metres; the XML carries bottom-left y (the loader flips it, bad_weather.py:221-222).  The
    image width max(iw1, iw2) picks the drop's type: >= 4 Big (bicubic warp of the texture onto tw = dx + floor(iw) by
    th = |dy|), else a rotated, resized texture."""
    fpx = cam['focal_mm'] * 1e-3 / (cam['pix_um'] * 1e-6)
    X = (x0 - W / 2) * depth / fpx
    Y = ((H - y0) - H / 2) * depth / fpx
    return dict(pid=pid, wp1=(X, Y, -depth), wp2=(X + 0.001, Y - 0.01, -depth + 0.005), wd1=0.002, wd2=0.002,
                ip1=(x0, H - y0), ip2=(x1, H - y1), iw1=iw1, iw2=iw2)


def oracle_render(scene, i, bg, rainy_bg, env_xyY, faithful=True, noise_std=0.0, noise_scale=0.0, max_drops=None, strategy=None,
                  first_drop=0, scene_depth=None):
    textures, ratio = scene.oracle_db()
    streaks = scene.oracle_streaks(i)
    return orc.render_frame(bg, rainy_bg, env_xyY, scene.omega, streaks, textures, ratio, scene.ocam, frame_seed=i,
                            noise_std=noise_std, noise_scale=noise_scale, faithful=faithful, max_drops=max_drops,
                            rendering_strategy=strategy, first_drop=first_drop, scene_depth=scene_depth)


def prepass_scene(H, W, seed, dtype=np.float32):
    """Seeded inputs of the pre-pass tests (image / 255 and a depth map in metres); tests/golden/make_golden_prepass.py
    feeds the same arrays to the reference."""
    bg = synthetic.make_frame(seed, H, W)
    rng = np.random.RandomState(seed)
    depth = (np.linspace(80, 2, H)[:, None] * np.ones((1, W)) + rng.uniform(0, 3, (H, W))).astype(dtype)
    return bg, depth
