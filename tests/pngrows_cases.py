"""Input files with CHOSEN scanline filter types for k_png_unfilter (csrc/rainhip.hip; the rule: csrc/rr_pngrows.h): a numpy forward
PNG filter, the sizes and the filter plans -- shared by tests/test_pngrows_cases_host.py (the filter on trial against the emulation
and PIL) and tests/test_gpu_pngrows_cases.py (the device against the ORIGINAL image and depth samples).

The kernel takes 64 rows at a time, lane l on row r0 + l one pixel behind lane l - 1; the row above a group of 64 comes through LDS
from lane 63 of the group before.  So the sizes put W below, at and above the 64-lane skew and H around one and two groups, and the
plans put every filter type on row 0 (no row above: Up, Average and Paeth see zeros), on rows 64 k - 1 (the lane that leaves the
row in LDS) and 64 k (the lane that takes it from there), in every ordered pair."""
import struct
import zlib

import numpy as np

TYPES = (0, 1, 2, 3, 4)                 # None, Sub, Up, Average, Paeth

# every W at H = 65 and every H at W = 65 (the pre-pass takes every positive size)
SIZES = [(65, 1), (65, 2), (65, 63), (65, 64), (65, 65), (1, 65), (63, 65), (64, 65), (128, 65), (129, 65)]


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def png_filter(raw, plan):
    """The filtered scanlines (H, 1 + bpp * W) of the samples raw (H, W, bpp) uint8 with filter type plan[y] on row y
    (PNG specification, section 9: the predictors read the UNFILTERED neighbours, 0 outside the image)."""
    H, W, bpp = raw.shape
    r = raw.astype(np.int64)
    left = np.zeros_like(r)
    left[:, 1:] = r[:, :-1]
    up = np.zeros_like(r)
    up[1:] = r[:-1]
    upl = np.zeros_like(r)
    upl[1:, 1:] = r[:-1, :-1]
    pred = np.stack([np.zeros_like(r), left, up, (left + up) >> 1, _paeth(left, up, upl)])
    plan = np.asarray(plan, np.int64)
    assert plan.shape == (H,) and plan.min() >= 0 and plan.max() <= 4
    rows = np.empty((H, 1 + bpp * W), np.uint8)
    rows[:, 0] = plan
    rows[:, 1:] = ((r - pred[plan, np.arange(H)]) & 255).astype(np.uint8).reshape(H, bpp * W)
    return rows


def image_samples(bgr):
    """The PNG sample order of the B G R image the device delivers: R G B."""
    return np.ascontiguousarray(bgr[..., ::-1])


def depth_samples(d16):
    """16-bit gray samples: big-endian byte pairs."""
    return np.stack([(d16 >> 8).astype(np.uint8), (d16 & 255).astype(np.uint8)], axis=-1)


def png_file(rows, W, H, depth16):
    """A PNG file around filtered scanlines: 8-bit RGB, or 16-bit gray."""
    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    ihdr = struct.pack('>IIBBBBB', W, H, 16 if depth16 else 8, 0 if depth16 else 2, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', ihdr) + chunk(b'IDAT', zlib.compress(np.ascontiguousarray(rows).tobytes())) + chunk(b'IEND', b'')


def plans(H, seed):
    """The filter plans of an H-row file: each type on every row; every ordered pair (a on rows 64 k - 1, b on rows 64 k) over a
    pseudo-random plan, where the file has such rows; two pseudo-random plans."""
    rng = np.random.RandomState(seed)
    out = [np.full(H, t, np.int64) for t in TYPES]
    if H > 64:
        for a in TYPES:
            for b in TYPES:
                p = rng.randint(0, 5, H)
                p[63::64] = a
                p[64::64] = b
                out.append(p)
    out += [rng.randint(0, 5, H), rng.randint(0, 5, H)]
    return out


_cache = {}


def batch(H, W):
    """The files of one size, made once and read-only: a list of dict(bgr, d16, image_plan, depth_plan, image_rows, depth_rows).
    File i carries plan i on its image and the plans in reverse order on its depth map (independent of each other); noise
    content, so Paeth's three-way choice and Average's carry are exercised."""
    if (H, W) not in _cache:
        rng = np.random.RandomState(1000 * H + W)
        ps = plans(H, H + W)
        files = []
        for i, p in enumerate(ps):
            bgr = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
            d16 = rng.randint(512, 20480, (H, W)).astype(np.uint16)          # 2 .. 80 m in 1/256 m: both bytes are noise
            q = ps[len(ps) - 1 - i]
            f = dict(bgr=bgr, d16=d16, image_plan=p, depth_plan=q, image_rows=png_filter(image_samples(bgr), p).ravel(),
                     depth_rows=png_filter(depth_samples(d16), q).ravel())
            for a in f.values():
                a.setflags(write=False)
            files.append(f)
        _cache[(H, W)] = files
    return _cache[(H, W)]
