"""The float64 reference of a frame's rain layer (csrc/rr_layer.h), from the renderers the suite already trusts.

Wherever no blend clamps, the composite is affine in the image it is blended over: composite = T rainy_bg + L, with T and L free
of rainy_bg.  So two renders of a compositor catalogue (tests/compositor_cases.py) over constant images give both:
    L = render(rainy_bg == 0),   T = (render(rainy_bg == 0.5) - L) / 0.5
with `bg` the case's own (it only enters the mean shift).  reference() checks on the reference alone that this holds for the
case -- both composites stay below 1 (nothing clamped: every blend keeps a value >= 0), a third render over 0.25 is reproduced
and T is the same in the three channels -- so the unchanged oracle and host build serve as they are.

The comparison bound of the GPU tier (bound()): the device carries T and L in float32; one step rounds Af, te, kg, the product
Af kg and two fma results, and with |1 - A te| <= 1 the error grows per step by at most 7 u max(1, |L|, |A kg|), u = 2^-24.  A
pixel that n listed drops' boxes hold is held to n 2^-21 max(1, max |L_ref|), plus the suite's 1e-9 for the float64 colour
constants."""
import numpy as np

import compositor_cases as cc
import helpers as h
from oracle import render as orc

HOST_BUILD = ('indices', 'segment_dim')      # tables the oracle would take minutes for (test_gpu_compositor_cases.py)
AFFINE_TOL = 1e-12


def segment_dim(tmp, tpl):
    """cc.segment's BIN_SEG + 40 records under a map dim enough for the stacks not to saturate (lum = 0.001: L <= 0.34)."""
    c = cc.Case('segment_dim', tmp, tpl, 40, 40, lum=0.001)
    cells = ((0, 0), (1, 0), (2, 2), (3, 2), (0, 3), (4, 4))
    stacks = [c.add_stack('cell_%d_%d' % cell, 0, 8 * cell[0], 8 * cell[1], ('segment',)) for cell in cells]
    for i in range(cc.BIN_SEG + 40):
        c.extend_stack(stacks[(i // 3) % len(stacks)], 1)
    return c.finish()


def _render(case, level, drops, depth):
    rainy = np.full_like(case.bg, level)
    if depth is not None or case.name in HOST_BUILD:
        return h.emu_render(case.scene, case.bg, rainy, case.env, drops, depth=depth)
    textures, _ = case.scene.oracle_db()
    return orc.render_drop_records(case.bg, rainy, case.env, case.scene.omega, drops, textures, case.scene.ocam, faithful=False)


def reference(case, depth=None, drops=None):
    """dict(L [H, W, 3] B G R, T [H, W], n [H, W] listed drops whose box holds the pixel, status, peak = the largest composite,
    affine = the error of the third render).  Asserts the condition under which L and T are the layer."""
    drops = case.drops if drops is None else drops
    r0, r5, r25 = (_render(case, v, drops, depth) for v in (0.0, 0.5, 0.25))
    L = r0['rainy_bg']
    T3 = (r5['rainy_bg'] - L) / 0.5
    T = T3.mean(axis=2)
    peak = max(float(L.max()), float(r5['rainy_bg'].max()))
    assert peak < 1.0, '%s: a composite reaches %.17g: a blend may have clamped' % (case.name, peak)
    spread = float(np.abs(T3 - T[..., None]).max())
    assert spread <= AFFINE_TOL, '%s: T differs between the channels by %.3g' % (case.name, spread)
    affine = float(np.abs(T[..., None] * 0.25 + L - r25['rainy_bg']).max())
    assert affine <= AFFINE_TOL, '%s: the render over 0.25 is missed by %.3g' % (case.name, affine)
    keep, boxes = cc.listed_drops(case.scene, drops, r0['status'])
    n = np.zeros((case.H, case.W), np.int64)
    for i in keep:
        x0, y0, x1, y1 = boxes[i]
        n[max(y0, 0):y1, max(x0, 0):x1] += 1
    return dict(L=L, T=T, n=n, status=r0['status'], peak=peak, affine=affine)


def bound(ref):
    """[H, W]: what the device's L (every channel) and T may differ from the reference by."""
    return ref['n'] * 2.0 ** -21 * max(1.0, float(np.abs(ref['L']).max())) + 1e-9
