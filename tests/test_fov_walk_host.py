"""CPU tier: k_fov_dda's polygon walk (rr_device.h fov_walk_make_records + FovWalk: the records as a chain per side, an edge
switch that takes a prepared record instead of deriving the edge) on the host build, tests/hostemu/fov_walk_emu.cpp.  Per
polygon and rule -- 0 the span rule (fov_rowspan), 1 OpenCV's (fov_rowspan_cv) where it applies -- the emulation makes the
records with the function the kernel's prologue calls, walks the rows top to bottom and counts the rows on which
(a <= b, a, b) differs from the rule; it counts the same for the walker before (DdaCursors).  Both are 0 everywhere."""
import ctypes
import importlib

import numpy as np
import pytest

import helpers as h
import test_fov_f32_host as f32host


@pytest.fixture(scope='module')
def emu():
    lib = ctypes.CDLL(importlib.import_module('__graft_entry__').build_emu('fovwalkemu'))
    lib.fov_walk_random.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def _bad(emu, px, py, He, We):
    """(rows off the rule: the new walk, DdaCursors) summed over both rules; (-1, -1): not monotone.  Rule 1 counts where it applies."""
    px, py = np.ascontiguousarray(px, np.int32), np.ascontiguousarray(py, np.int32)
    new = old = 0
    for rule in (0, 1):
        o = ctypes.c_int32(-7)
        b = emu.fov_walk_check(h._p(px), h._p(py), len(px), He, We, rule, ctypes.byref(o))
        if b < 0:
            assert o.value == -1
            if rule == 0:
                return -1, -1
            continue
        new, old = new + b, old + o.value
    return new, old


def _every_way_round(px, py):
    """the vertex list in every rotation and both orientations"""
    px, py = list(px), list(py)
    for qx, qy in ((px, py), (px[::-1], py[::-1])):
        for r in range(len(px)):
            yield qx[r:] + qx[:r], qy[r:] + qy[:r]


def test_scene_polygons(tmp_path, emu):
    """the 20-gons (and the few wrapping 24-gons: not monotone, -1) of a KITTI and a wide-angle scene, float64 and float32 vertices"""
    n_checked = n_general = 0
    for cam, H, W in ((h.KITTI, 375, 1242), (h.NUSCENES, 450, 800)):
        sc = h.Scene(tmp_path / ('s%d' % H), H, W, 3000, cam=cam, seed0=5300, far_fraction=0.2)
        drops, p64, n64, p32, n32, used, ratio, off = f32host._polygons(sc, 0)
        for P, Nn in ((p64, n64), (p32, n32)):
            for k in range(len(drops)):
                if Nn[k] > 0:
                    new, old = _bad(emu, P[k, 0, :Nn[k]], P[k, 1, :Nn[k]], sc.He, sc.We)
                    if new < 0:
                        n_general += 1
                    else:
                        assert (new, old) == (0, 0), (k, P[k, :, :Nn[k]])
                        n_checked += 1
                    if Nn[k] == 20:
                        assert new == 0, "a 20-gon that is not monotone: %r" % (P[k, :, :20],)
    assert n_checked > 4000 and n_general < 0.05 * n_checked


@pytest.mark.parametrize("He,We,border,trials", [(375, 1909, 1, 6000), (375, 1909, 0, 6000), (64, 128, 1, 6000), (64, 128, 0, 6000),
                                                 (1024, 4096, 0, 8000)])
def test_random_monotone_polygons_with_ties(emu, He, We, border, trials):
    """32 000 in all, the loop in C++.  border 1: vertices on row He and column We as test_thread_per_drop_spans_equal_the_rule's
    generator makes them (OpenCV's rule does not apply to those); 0: every vertex on the map, so both rules walk every polygon.
    1024 x 4096 is the largest map of the fast colour path, on the map only: den <= 1023 and |dx| <= 4095 are the records' limits."""
    out = np.zeros(7, np.int64)
    assert emu.fov_walk_random(5 + He, trials, He, We, border, h._p(out)) == 0
    n0, n1, bad_new, bad_old, not_monotone, den, dx = (int(v) for v in out)
    assert not_monotone == 0 and n0 == trials
    assert n1 == trials if not border else 0 < n1 < trials
    assert (bad_new, bad_old) == (0, 0)
    assert den <= 1023 and dx <= 4095                          # (test_edges_at_the_records_limits has den = 1023 and |dx| = 4095 themselves)


HE, WE = 64, 128
HAND_MADE = {
    'all on one row': ([5, 90, 40], [7, 7, 7]),
    'all on one row, five': ([5, 90, 40, 41, 3], [7, 7, 7, 7, 7]),
    'flat top and bottom of three': ([10, 20, 30, 40, 25, 5], [3, 3, 3, 20, 20, 20]),
    'flat top and bottom of four and five': ([10, 20, 30, 35, 60, 40, 25, 12, 5], [3, 3, 3, 3, 9, 20, 20, 20, 20]),
    'flat top wider than what follows': ([50, 10, 90, 60, 40], [5, 5, 5, 30, 30]),
    'two vertices on one row in mid-side': ([30, 50, 70, 60, 30, 10, 5], [2, 10, 10, 40, 40, 25, 25]),
    'three on one row in mid-side, going back': ([30, 50, 90, 70, 60, 20], [2, 10, 10, 10, 40, 30]),
    'den = 1 runs on both sides at once': ([60, 70, 85, 86, 120, 100, 40, 20, 30, 10, 50], [0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1]),
    'den = 1 runs, steep and shallow': ([60, 61, 61, 62, 100, 58, 20, 57, 59], [10, 11, 12, 13, 14, 15, 13, 12, 11]),
    'repeated vertices': ([3, 3, 8, 8, 8], [2, 2, 2, 9, 9]),
    'repeated vertices at the bottom and in mid-side': ([30, 50, 50, 40, 40, 10, 10], [1, 8, 8, 30, 30, 12, 12]),
    'rows 0 and He - 1': ([5, 9, 9, 5], [0, 0, HE - 1, HE - 1]),
    'rows 0 and He': ([5, 9, 9, 5], [0, 0, HE, HE]),
    'rows He - 1 and He': ([5, 100, 60], [HE - 1, HE - 1, HE]),
    'a vertex on column We': ([5, WE, 60], [3, 20, 40]),
    'a triangle': ([40, 90, 10], [5, 30, 50]),
    'a triangle with a flat top': ([40, 90, 60], [5, 5, 50]),
    'a triangle with a flat bottom': ([40, 90, 10], [5, 50, 50]),
    'bottom reached by both sides on one row, one through a horizontal edge': ([40, 80, 60, 20, 10], [5, 30, 50, 50, 30]),
    'the same, the other side': ([40, 80, 100, 60, 10], [5, 30, 50, 50, 30]),
    'bottom through horizontal edges from both sides': ([40, 80, 90, 60, 30, 10], [5, 30, 50, 50, 50, 30]),
    'one row high': ([10, 50, 60, 5], [7, 7, 8, 8]),
    'a sliver of two rows': ([10, 100, 11], [7, 8, 8]),
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_polygons_every_way_round(emu, name):
    px, py = HAND_MADE[name]
    n = 0
    for qx, qy in _every_way_round(px, py):
        for He, We in ((HE, WE), (375, 1909)):
            assert _bad(emu, qx, qy, He, We) == (0, 0), (name, qx, qy, He, We)
            n += 1
    assert n == 4 * len(px)


AT_THE_LIMITS = {
    'den = 1023 with dx = 4095, flat bottom': ([0, 4095, 0], [0, 1023, 1023]),
    'den = 1023 with dx = -4095, flat bottom': ([4095, 4095, 0], [0, 1023, 1023]),
    'den = 1023 on both sides, flat top': ([0, 4095, 2000], [0, 0, 1023]),
    'den = 1 with |dx| = 4095: 2047 pixels either way': ([0, 4095, 0], [500, 501, 502]),
    'den = 1 with |dx| = 4095 on both sides': ([4095, 4095, 0, 0], [1021, 1022, 1023, 1022]),
    'den = 1022 and 1: a remainder one short of 2 den': ([0, 4095, 4095, 1], [0, 1022, 1023, 1023]),
}


@pytest.mark.parametrize("name", sorted(AT_THE_LIMITS))
def test_edges_at_the_records_limits(emu, name):
    """1024 x 4096, the largest map of the fast colour path: den = 1023 (10 bits), 2 den = 2046 and hh = 2047 (11 bits), |dx| = 4095"""
    px, py = AT_THE_LIMITS[name]
    for qx, qy in _every_way_round(px, py):
        assert _bad(emu, qx, qy, 1024, 4096) == (0, 0), (name, qx, qy)


def test_not_monotone_is_not_walked(emu):
    assert _bad(emu, [0, 50, 20, 70, 10], [0, 40, 10, 40, 80], 375, 1909) == (-1, -1)        # up and down twice
