"""The scenes of the lens tests (tests/test_lens_host.py on the CPU, tests/test_gpu_lens_drops.py on the device): frames of 61 x 47
pixels -- width and planes odd, so every plane but the first is misaligned -- n = 3 with 8, 0 and 1 drops, and one wider frame
whose single drop spans three sub-tiles.  Between them the drops cover: rx = ry = 0.75 (a pixel or two); a box clipped at each of the
four edges and at a corner; rx > W (the whole frame: 2 x 2 sub-tiles); ry = 2 rx; blur classes of radius 0, 4 and 15; mag 1 and 8
(the samples clamp at the borders); edge 1 and 0.1; rim 0 and 1.  The statement's results are computed once (functools.lru_cache)."""
import functools
import importlib

import numpy as np

lens = importlib.import_module('rain-rendering_amd.tools.lens')

H, W = 47, 61
WEIGHTS = lens.blur_table([0.0, 1.2, 5.0])              # radii 0, 4, 15
assert list(WEIGHTS[0]) == [0, 4, 15]


def _rec(*rows):
    t = np.zeros(len(rows), lens.LENS_DROP_DTYPE)
    for i, r in enumerate(rows):
        t[i] = r
    return t


#         cx    cy    rx    ry   mag  edge  rim  class
FRAME0 = _rec(
    (30.3, 23.6, 0.75, 0.75, 1.0, 1.0, 0.0, 0),         # at most a pixel or two
    (1.0, 10.0, 4.0, 4.0, 8.0, 0.1, 1.0, 2),            # clipped at the left edge; radius 15, mag 8, a small edge, rim 1
    (20.0, 0.5, 5.0, 5.0, 3.0, 0.3, 0.4, 1),            # clipped at the top
    (59.5, 25.0, 4.0, 8.0, 5.0, 0.2, 0.6, 1),           # clipped at the right edge; ry = 2 rx
    (30.0, 45.5, 6.0, 6.0, 4.0, 1.0, 0.2, 2),           # clipped at the bottom; edge 1
    (1.5, 45.0, 5.0, 5.0, 6.0, 0.25, 0.5, 0),           # clipped at a corner; radius 0
    (42.0, 12.0, 7.0, 9.0, 8.0, 0.15, 0.0, 2),          # mag 8, rim 0, radius 15
    (14.0, 28.0, 8.0, 8.5, 1.0, 0.4, 1.0, 1),           # mag 1, rim 1
)
FRAME2 = _rec((30.0, 23.0, 62.0, 40.0, 3.0, 0.6, 0.5, 1))       # rx > W: the whole frame, four work items
TABLES = [FRAME0, _rec(), FRAME2]

WIDE_H, WIDE_W = 37, 101
WIDE_TABLES = [_rec((50.5, 18.0, 45.0, 16.0, 2.0, 0.3, 0.7, 2))]         # 92 x 34 pixels: three sub-tiles across, two down; radius 15


def images(n, h, w, dtype, seed=5):
    """Planar [n, 3, h, w]: a smooth ramp plus noise, bytes or float32 in [0, 1] with full mantissas."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * (c + 1) + y * (3 - c)) % 97 / 96.0 for c in range(3)])[None] * 0.7
    v = np.clip(base + 0.3 * rs.random_sample((n, 3, h, w)), 0.0, 1.0)
    return (v * 255.0).astype(np.uint8) if dtype == np.uint8 else v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name, dtype_name):
    """(images, tables, the statement's output, the statement's alpha) of scene 'odd' or 'wide' for dtype 'uint8' / 'float32'."""
    dtype = np.dtype(dtype_name).type
    tabs, (h, w) = (TABLES, (H, W)) if name == 'odd' else (WIDE_TABLES, (WIDE_H, WIDE_W))
    img = images(len(tabs), h, w, dtype)
    out, alpha = lens.apply_numpy(img, tabs, WEIGHTS, alpha=True)
    for a in (img, out, alpha):
        a.setflags(write=False)
    return img, tabs, out, alpha


SCENES = [(s, d) for s in ('odd', 'wide') for d in ('uint8', 'float32')]
