"""The catalogue of output files with CHOSEN scanline bytes that pins the device's PNG entropy coder (k_pngz_blocks / k_pngz_pack,
csrc/rr_deflate.h) at its edges -- shared by the CPU tier (tests/test_pngz_cases_host.py: the catalogue and the emulation on trial)
and the GPU tier (tests/test_gpu_pngz_cases.py: the catalogue through the C ABI).

How a case reaches the coder.  A frame without drops leaves image_u8 = trunc(rainy_bg * 255); rainy_bg = (k + 0.5) / 255 gives the
byte k back (float64 and float32, all 256 bytes: checked in the CPU tier).  k_png_image then writes, per row, the filter byte 1 and
the Sub-filtered RGBA pixels (alpha 255: the alpha byte is 255 at x = 0 and 0 behind it).  So for wanted Sub-filtered RGB bytes
F[y, x, c] the image is cumsum_x(F) mod 256 and the scanlines are `intended(F)`; three of every four bytes are free.

What stays with the CPU tier (tests/test_deflate_hostemu.py): a 32 KB block that is STORED in the middle of a file.  Through the
ABI every fourth byte of a block is the alpha difference 0, and uniformly random RGB bytes around them still code at 0.86 n, so no
image makes a full block incompressible; only raw scanline bytes can, and no entry point takes those.

A file of n = H (1 + 4 W) bytes is cut into blocks of 32768 bytes, a block into eight eighths of 4096 bytes (one wave each), an eighth
into chunks of 64 bytes (one lane per byte).  The sizes below are factorisations of the n that put the file's end where the coder
can go wrong; `lands` says where, and the CPU tier asserts it on the emulation's trace (emu_pngz_trace).
"""
import collections
import ctypes
import heapq

import numpy as np

import helpers as h

BLOCK, EIGHTH, CHUNK, HEADER = 32768, 4096, 64, 16
MAGIC = b'RRZ1'

# tests/hostemu/hostemu.cpp PngzTrace: one record per block
PNGZ_TRACE_DTYPE = np.dtype([(k, '<i4') for k in 'stored bytes len nlit max_len kraft_changed depth cut_chunk cut_eighth cut_block'.split()] +
                            [('chunks', '<i4', (8,)), ('seqs', '<i4', (65,)), ('pad_', '<i4'), ('runs', '<i4', (64, 64))])


def emu_pngz(rows, trace=False):
    """(length of the zlib stream or 0, the n bytes the device leaves in the file's buffer[, trace records]) by the host build of
    rr_deflate.h."""
    emu = h.hostemu()
    rows = np.ascontiguousarray(rows, np.uint8).ravel()
    dst = np.zeros_like(rows)
    if not trace:
        emu.emu_pngz.restype = ctypes.c_int64
        emu.emu_pngz.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        return int(emu.emu_pngz(rows.ctypes.data, rows.size, dst.ctypes.data)), dst
    tr = np.zeros((rows.size + BLOCK - 1) // BLOCK, PNGZ_TRACE_DTYPE)
    emu.emu_pngz_trace.restype = ctypes.c_int64
    emu.emu_pngz_trace.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    total = int(emu.emu_pngz_trace(rows.ctypes.data, rows.size, dst.ctypes.data, tr.ctypes.data, PNGZ_TRACE_DTYPE.itemsize))
    assert total >= 0, "PNGZ_TRACE_DTYPE is not hostemu.cpp's PngzTrace"
    return total, dst, tr


# ---- images from scanline bytes and back ------------------------------------------------------------------------------------------
def image_of(F):
    """The RGB image whose Sub-filtered bytes are F (H, W, 3)."""
    return (np.cumsum(F.astype(np.int64), axis=1) & 255).astype(np.uint8)


def rainy_bg_of(img_rgb):
    """The BGR float64 background that a frame without drops turns back into img_rgb."""
    return np.ascontiguousarray((img_rgb[..., ::-1].astype(np.float64) + 0.5) / 255.0)


def scanlines_rgba(rgba):
    """numpy's Sub filter of an RGBA image: the filter byte 1 and the byte-wise differences to the pixel on the left."""
    H, W, _ = rgba.shape
    d = rgba.astype(np.int16)
    d[:, 1:] -= rgba[:, :-1].astype(np.int16)
    rows = np.empty((H, 1 + 4 * W), np.uint8)
    rows[:, 0] = 1
    rows[:, 1:] = (d & 255).astype(np.uint8).reshape(H, 4 * W)
    return rows.ravel()


def scanlines_rgb(img_rgb):
    """k_png_image's file of an RGB image: alpha 255."""
    return scanlines_rgba(np.concatenate([img_rgb, np.full(img_rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1))


def intended(F):
    """The scanline bytes a case aims at: F between the bytes k_png_image fixes."""
    H, W, _ = F.shape
    px = np.zeros((H, W, 4), np.uint8)
    px[..., :3] = F
    px[:, 0, 3] = 255
    rows = np.empty((H, 1 + 4 * W), np.uint8)
    rows[:, 0] = 1
    rows[:, 1:] = px.reshape(H, 4 * W)
    return rows.ravel()


def mask_rgba(mask, lut):
    """The host writer's rule for the mask file (common/imgops.imsave_scalar, generator.py:467) with the colour map `lut`."""
    a = np.asarray(mask, np.float64)
    lo, hi = float(a.min()), float(a.max())
    norm = np.zeros_like(a) if hi <= lo else (a - lo) / (hi - lo)
    return np.ascontiguousarray(lut[np.clip((norm * 256).astype(np.int64), 0, 255)])


def random_lut(seed=5):
    """A colour map of 256 distinct RGBA entries, alpha varied: the mask file's bytes are not nearly constant."""
    rng = np.random.RandomState(seed)
    lut = rng.randint(0, 256, (256, 4)).astype(np.uint8)
    lut[:, 0] = rng.permutation(256)                      # (distinct whatever the other three draw)
    return lut


# ---- contents ---------------------------------------------------------------------------------------------------------------------
def huffman_depth(counts):
    """Depth of the deepest leaf of an unrestricted Huffman tree over `counts` (a heap construction; ties: lighter, then older)."""
    heap = [(int(c), i, 0) for i, c in enumerate(counts) if c > 0]
    heapq.heapify(heap)
    tick = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return heap[0][2]


def _chain(free, fixed):
    """Leaf counts, ascending, of the longest chain in which every Huffman merge takes the node merged so far (so the tree is a
    spine: depth = leaves - 1): leaf k + 1 must outweigh everything merged before leaf k.  `fixed`: counts the file's format
    dictates (the end-of-block symbol, the filter byte, the alpha bytes), all of which must appear; the other leaves use at most
    `free` bytes, the last one whatever is left.  Returns [(count, is_fixed)]."""
    fixed = sorted(fixed)
    best = []

    def go(leaves, acc_prev, acc, fi, used):
        nonlocal best
        need = max(leaves[-1][0], acc_prev + 1)            # the least the next leaf may weigh
        if fi == len(fixed) and free - used >= need and len(leaves) + 1 > len(best):
            best = leaves + [(free - used, False)]        # close the chain with the rest of the bytes
        if fi < len(fixed) and fixed[fi] >= need:
            go(leaves + [(fixed[fi], True)], acc, acc + fixed[fi], fi + 1, used)
        if used + need <= free and (fi == len(fixed) or need <= fixed[fi]):
            go(leaves + [(need, False)], acc, acc + need, fi, used + need)

    assert fixed[0] == 1                                   # the end-of-block symbol opens the chain
    go([(1, True)], 0, 1, 1, 0)
    return best


def deep_F(H, W, seed):
    """Sub-filtered RGB bytes whose FIRST block has a histogram like 1, 2, 3, 5, ...: the end-of-block symbol is the leading 1, the
    bytes the format fixes (filter 1, alpha 255 and 0) take their places in the chain, and no byte value repeats four times in a row
    (values 2..254 between alpha bytes), so no length symbol disturbs it.  The unrestricted tree is deeper than 15."""
    rng = np.random.RandomState(seed)
    rows = intended(np.full((H, W, 3), 7, np.uint8)).reshape(H, 1 + 4 * W)
    free_mask = np.zeros_like(rows, bool)
    free_mask[:, 1:] = (np.arange(4 * W) % 4 != 3)[None, :]
    flat_free = np.flatnonzero(free_mask.ravel())
    in0 = flat_free[flat_free < BLOCK]
    first = rows.ravel()[:BLOCK]
    fixed = [1] + [int(np.sum((first == v) & ~free_mask.ravel()[:BLOCK])) for v in (1, 255, 0)]
    chain = _chain(len(in0), fixed)
    counts = [c for c, is_fixed in chain if not is_fixed]
    values = rng.permutation(np.arange(2, 255))[:len(counts)]
    fill = np.repeat(values, counts).astype(np.uint8)
    rng.shuffle(fill)
    out = rows.ravel().copy()
    out[flat_free] = values[-1]                            # (the bytes behind the first block: the commonest value)
    out[in0] = fill
    return out.reshape(H, 1 + 4 * W)[:, 1:].reshape(H, W, 4)[..., :3].copy()


def sparse_F(H, W, seed):
    """Stretches of 1..27 non-zero bytes between zero runs of 1..130 bytes (about 0.7 of the bytes zero), laid over the scanlines
    and not over the rows: runs of every length begin at every lane and are cut by whatever edge comes."""
    rng = np.random.RandomState(seed)
    n = H * (1 + 4 * W)
    s = np.zeros(n, np.uint8)
    i = 0
    while i < n:
        k = min(int(rng.randint(1, 48)), n - i)
        s[i:i + k] = rng.randint(1, 256, k)
        i += k + (int(rng.randint(1, 67)) if rng.randint(0, 4) else int(rng.randint(60, 131)))
    return s.reshape(H, 1 + 4 * W)[:, 1:].reshape(H, W, 4)[..., :3].copy()


def content(kind, H, W, seed):
    """F (H, W, 3) uint8 of a case."""
    rng = np.random.RandomState(seed)
    if kind == 'random':
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == 'sparse':
        return sparse_F(H, W, seed)
    if kind == 'flat':
        return np.zeros((H, W, 3), np.uint8)
    if kind == 'nozero':
        return rng.randint(1, 256, (H, W, 3)).astype(np.uint8)
    if kind == 'ff':
        return np.full((H, W, 3), 255, np.uint8)
    if kind == 'deep':
        return deep_F(H, W, seed)
    raise ValueError(kind)


Case = collections.namedtuple('Case', 'name H W kind seed lands')


def _n(H, W):
    return H * (1 + 4 * W)


# Files too small to shrink, and the threshold: uniformly random RGB, rising size.  The emulation finds the neighbours between
# which "kept as scanlines" turns into "coded" (threshold_pair); the CPU tier asserts that everything below is kept and everything
# above coded.
LADDER = [(1, 1), (2, 3), (5, 7), (8, 8), (11, 13), (13, 16), (14, 16), (15, 16), (16, 16), (16, 17), (17, 18), (24, 24)]

# (H, W, what the size is for, {block: (stored, len)} of the blocks named, waves that have nothing to do in the last block)
EDGES = [
    (151, 54, 'n = 32767: one block, one byte short', {0: (0, 32767)}, 0),
    (9, 910, 'n = 32769: a last block of ONE byte', {0: (0, 32768), 1: (1, 1)}, 7),
    (64, 128, 'n = 32832: a last block of exactly one chunk', {0: (0, 32768), 1: (1, 64)}, 7),
    (21, 780, 'n = 65541: three blocks, the last of five bytes', {0: (0, 32768), 1: (0, 32768), 2: (1, 5)}, 7),
    (74, 27, 'n = 8066: the file ends 2 bytes into a chunk', {0: (0, 8066)}, 6),
    (47, 43, 'n = 8131: ... 3 bytes into a chunk', {0: (0, 8131)}, 6),
    (43, 47, 'n = 8127: ... 63 bytes into a chunk', {0: (0, 8127)}, 6),
    (191, 48, 'n = 36863: the last block one short of an eighth', {0: (0, 32768), 1: (0, 4095)}, 7),
    (4096, 2, 'n = 36864: the last block exactly an eighth', {0: (0, 32768), 1: (0, 4096)}, 7),
    (101, 91, 'n = 36865: the last block one past an eighth', {0: (0, 32768), 1: (0, 4097)}, 6),
]

CASES = [Case('ladder-%dx%d' % hw, hw[0], hw[1], 'random', 0, None) for hw in LADDER]
for H_, W_, why, blocks, idle in EDGES:
    for kind in ('sparse', 'flat'):
        CASES.append(Case('edge-%dx%d-%s' % (H_, W_, kind), H_, W_, kind, 1, dict(why=why, blocks=blocks, idle=idle)))
CASES += [
    Case('runs-sparse-a', 21, 780, 'sparse', 2, None),
    Case('runs-sparse-b', 21, 780, 'sparse', 3, None),
    Case('nozero', 64, 128, 'nozero', 4, None),
    Case('adler-ff', 64, 128, 'ff', 0, None),
    Case('limit-15', 64, 128, 'deep', 6, None),
    Case('random-block', 64, 128, 'random', 7, None),
]
RUN_CASES = [c for c in CASES if c.kind in ('sparse', 'flat')]
assert all(_n(c.H, c.W) <= 72000 for c in CASES)


def by_name(name):
    return next(c for c in CASES if c.name == name)


def sizes():
    """The frame sizes of the catalogue, each with its cases (one batch per size on the device)."""
    out = collections.OrderedDict()
    for c in CASES:
        out.setdefault((c.H, c.W), []).append(c)
    return out


_cache = {}


def built(case):
    """(F, image RGB, intended scanlines) of a case, made once and read-only."""
    if case.name not in _cache:
        F = content(case.kind, case.H, case.W, case.seed)
        img = image_of(F)
        rows = intended(F)
        for a in (F, img, rows):
            a.setflags(write=False)
        _cache[case.name] = (F, img, rows)
    return _cache[case.name]


def threshold_pair():
    """The neighbours of LADDER between which the emulation turns from keeping the scanlines to coding them: (index kept, index coded)."""
    kept = [emu_pngz(built(by_name('ladder-%dx%d' % hw))[2])[0] == 0 for hw in LADDER]
    k = kept.index(False)
    return k - 1, k, kept
