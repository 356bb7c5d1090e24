"""The catalogue of the input-resize kernels (k_resize_in<KIND> / k_resize_depth<KIND>, one body: resize_rows in csrc/rainhip.hip;
DESIGN.md 5o), aimed at the body's branch points: segments behind the first, the staged / direct choice at its limit, every kind's
LDS geometry, the buffer-end windows and the three store shapes.  tests/resize_cases.py stays what it was (nine one-segment sizes);
this module is shared by tests/test_input_resize_catalogue_host.py (the census and the g++ build of the header) and
tests/test_gpu_input_resize_catalogue.py (the kernels through rr_resize_inputs_device).

predict() restates the launch arithmetic on the host, so that what a case reaches is a property of its sizes, decided before any
device runs.  The reference of every comparison is common/imgops.py resize_linear on the float64 values of the input, compared as
bit patterns."""
import collections
import importlib
import math
import os
import re

import numpy as np

import helpers as h

imgops = importlib.import_module('rain-rendering_amd.common.imgops')
hb = h.hb

N = 3           # frames per case: the first, a middle and the last frame of the buffer


def _hip_constant(name):
    src = open(os.path.join(h.ROOT, 'rain-rendering_amd', 'csrc', 'rainhip.hip')).read()
    m = re.search(r'constexpr int %s = ([^;,]+)[;,]' % name, src)
    assert m, name
    return int(np.prod([int(v) for v in m.group(1).split('*')]))      # `256` / `6 * 6656`


RSZ_THREADS = _hip_constant('RSZ_THREADS')      # `constexpr int RSZ_THREADS = 256, RSZ_SEG = 2 * RSZ_THREADS;`
RSZ_SEG = 2 * RSZ_THREADS
RSZ_POOL = _hip_constant('RSZ_POOL')            # `constexpr int RSZ_POOL = 6 * 6656;`

Kind = collections.namedtuple('Kind', 'code image EL P el planar rgb half')
# EL (bytes per pixel of a piece) and P (pieces per source row) restate resize_rows:
#   P  = (KIND == RSZ_RGB8P || KIND == RSZ_RGBF32P || KIND == RSZ_RGBF16P || KIND == RSZ_RGBBF16P) ? 3 : 1
#   EL = (KIND == RSZ_BGR8 || KIND == RSZ_RGB8I) ? 3 : (KIND == RSZ_RGB8P ? 1 : (KIND == RSZ_RGBF32I ? 12 :
#        (HALF ? (P == 3 ? 2 : 6) : (KIND == RSZ_D16 ? 2 : 4))))
# el: bytes per element; rgb: the channel order in memory is R G B (the output is B G R); half: 'f16' / 'bf16' / None
KINDS = collections.OrderedDict([
    ('bgr_u8', Kind(hb.RR_RESIZE_BGR_U8, True, 3, 1, 1, False, False, None)),                    # RSZ_BGR8:     EL 3, P 1
    ('rgb_u8_planar', Kind(hb.RR_RESIZE_RGB_U8_PLANAR, True, 1, 3, 1, True, True, None)),        # RSZ_RGB8P:    EL 1, P 3
    ('rgb_f32_planar', Kind(hb.RR_RESIZE_RGB_F32_PLANAR, True, 4, 3, 4, True, True, None)),      # RSZ_RGBF32P:  EL 4, P 3
    ('rgb_u8', Kind(hb.RR_RESIZE_RGB_U8, True, 3, 1, 1, False, True, None)),                     # RSZ_RGB8I:    EL 3, P 1
    ('rgb_f32', Kind(hb.RR_RESIZE_RGB_F32, True, 12, 1, 4, False, True, None)),                  # RSZ_RGBF32I:  EL 12, P 1
    ('rgb_f16_planar', Kind(hb.RR_RESIZE_RGB_F16_PLANAR, True, 2, 3, 2, True, True, 'f16')),     # RSZ_RGBF16P:  EL 2, P 3
    ('rgb_bf16_planar', Kind(hb.RR_RESIZE_RGB_BF16_PLANAR, True, 2, 3, 2, True, True, 'bf16')),  # RSZ_RGBBF16P: EL 2, P 3
    ('rgb_f16', Kind(hb.RR_RESIZE_RGB_F16, True, 6, 1, 2, False, True, 'f16')),                  # RSZ_RGBF16I:  EL 6, P 1
    ('rgb_bf16', Kind(hb.RR_RESIZE_RGB_BF16, True, 6, 1, 2, False, True, 'bf16')),               # RSZ_RGBBF16I: EL 6, P 1
    ('u16', Kind(hb.RR_DEPTH_U16, False, 2, 1, 2, False, False, None)),                          # RSZ_D16:      EL 2, P 1
    ('f32', Kind(0, False, 4, 1, 4, False, False, None)),                                        # RSZ_DF32:     EL 4, P 1
])
IMAGE_KINDS = tuple(k for k, v in KINDS.items() if v.image)
DEPTH_KINDS = ('u16', 'f32')
BYTE_KINDS = ('bgr_u8', 'rgb_u8_planar', 'rgb_u8')
CLASS_NAMES = {(3, 1, True): 'bytes interleaved', (1, 3, True): 'bytes planar', (4, 3, True): 'float32 planar', (12, 1, True): 'float32 interleaved',
               (2, 3, True): 'half planar', (6, 1, True): 'half interleaved', (2, 1, False): 'uint16 depth', (4, 1, False): 'float32 depth'}


def kind_class(kind):
    k = KINDS[kind]
    return CLASS_NAMES[(k.EL, k.P, k.image)]


def cap(kind):
    """`constexpr int CAP = RSZ_POOL / (2 * P);`: the LDS bytes of one piece."""
    return RSZ_POOL // (2 * KINDS[kind].P)


def span_limit(kind):
    """The widest source span (columns) that `staged = (xb - xa + 1) * EL + 30 <= CAP` still stages."""
    return (cap(kind) - 30) // KINDS[kind].EL


def resize_coord(k, s, scale):
    """rrresize::resize_coord: (i0, i1, w) of destination index k on a source axis of length s."""
    f = (k + 0.5) * scale - 0.5
    fl = math.floor(f)
    w = 0.0 if fl < 0 else f - fl
    return min(max(fl, 0), s - 1), min(max(fl + 1, 0), s - 1), w


Segment = collections.namedtuple('Segment', 'xs xe xa xb span staged')
Prediction = collections.namedtuple('Prediction', 'grid segments residues stores tail unaligned')


def predict(kind, H, W, sH, sW, base_offset=0, n=N, out_offset=0):
    """What one launch of resize_rows<kind> does, from its sizes alone.
    grid: (segments, rows, frames).  segments: per blockIdx.x its xs, xe (destination columns [xs, xe)), xa, xb (source columns it
    reads), span = xb - xa + 1 and whether it is staged in LDS.  residues: the set of (address & 15) of the first byte of every
    piece any workgroup stages or reads (frame, row pair, plane, segment), the buffer starting base_offset bytes past a 16-byte
    boundary.  stores: {(frame, row): shape} of the lanes' two-pixel stores -- image '16' (three 16-byte stores) / '8off' (8 + 16 +
    16 + 8), depth 'pair' (one 8-byte store) / 'single' (two dwords) -- the output starting out_offset bytes past a 16-byte boundary.
    tail: a row ends in a one-pixel store (odd W).  unaligned: the buffer does not start on a 16-byte boundary."""
    k = KINDS[kind]
    sx, sy = sW / W, sH / H
    segs = []
    for b in range((W + RSZ_SEG - 1) // RSZ_SEG):
        xs, xe = b * RSZ_SEG, min(b * RSZ_SEG + RSZ_SEG, W)
        xa, xb = resize_coord(xs, sW, sx)[0], resize_coord(xe - 1, sW, sx)[1]
        segs.append(Segment(xs, xe, xa, xb, xb - xa + 1, (xb - xa + 1) * k.EL + 30 <= cap(kind)))
    row_bytes = sW * k.EL
    plane_bytes = row_bytes * sH
    stride = sH * sW * 3 * k.el if k.image else sH * sW * k.el          # the entry point's frame stride
    residues = set()
    for f in range(n):
        for y in range(H):
            y0, y1, _ = resize_coord(y, sH, sy)
            for yy in (y0, y1):
                for p in range(k.P):
                    for s in segs:
                        residues.add((base_offset + f * stride + (2 - p) * plane_bytes * (k.P == 3) + yy * row_bytes + s.xa * k.EL) & 15)
    stores = {}
    for f in range(n):
        for y in range(H):
            px = f * H * W + y * W
            if k.image:
                stores[(f, y)] = '16' if (out_offset + px * 24) & 15 == 0 else '8off'
            else:
                stores[(f, y)] = 'pair' if (out_offset + px * 4) & 7 == 0 else 'single'
    return Prediction((len(segs), H, n), segs, residues, stores, W % 2 == 1, base_offset % 16 != 0)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'name group kind H W sH sW offset reason')
CASES = collections.OrderedDict()


def _add(name, group, kind, dst, src, reason, offset=0):
    assert name not in CASES, name
    CASES[name] = Case(name, group, kind, dst[0], dst[1], src[0], src[1], offset, reason)


# segment counts: a down-sample by 2 for every kind
for _kind in KINDS:
    _add('seg513-' + _kind, 'segments', _kind, (3, 513), (6, 1026), 'a last segment of one pixel: blockIdx.x = 1 makes the tail store alone')
    _add('seg1024-' + _kind, 'segments', _kind, (2, 1024), (4, 2048), 'two full segments: xs = 512, xa > 0, an LDS window that starts inside a row')
    _add('seg1025-' + _kind, 'segments', _kind, (5, 1025), (10, 2050), 'two full segments and one pixel: three workgroups per row')
for _kind in ('rgb_u8', 'rgb_f32', 'rgb_f16_planar', 'u16'):      # EL 3, 12, 2 (planes) and 2
    _add('segfrac-' + _kind, 'segments', _kind, (4, 1025), (7, 2049), 'a fractional ratio over three segments: weights and window starts differ per segment')


def first_direct_width(kind, W=520, sH=3, H=2):
    """The smallest source width whose first 512-pixel segment of a W-wide destination no longer fits the pool."""
    sW = W
    while predict(kind, H, W, sH, sW, n=1).segments[0].staged:
        sW += 1
    return sW


# staging limit: W = 520 (a 512-pixel segment on one side of the limit and an 8-pixel segment that is staged); odd source heights
_LIMIT_SH = {'bgr_u8': 3, 'rgb_u8_planar': 5, 'rgb_f32_planar': 3, 'rgb_u8': 5, 'rgb_f32': 3, 'rgb_f16_planar': 5, 'rgb_bf16_planar': 3,
             'rgb_f16': 3, 'rgb_bf16': 5, 'u16': 3, 'f32': 5}
LIMIT_WIDTHS = {}
for _kind in KINDS:
    _sh = _LIMIT_SH[_kind]
    _w = first_direct_width(_kind, 520, _sh, 2)
    LIMIT_WIDTHS[_kind] = (_w - 1, _w)
    _add('limit-staged-' + _kind, 'limit', _kind, (2, 520), (_sh, _w - 1), 'the widest first segment that is still staged: its pieces fill their LDS regions to the end')
    _add('limit-direct-' + _kind, 'limit', _kind, (2, 520), (_sh, _w), 'one source column more: segment 0 reads global memory, segment 1 stays staged')

# shapes, each for a byte kind, float kinds of both layouts, and both depth kinds
_SHAPE_KINDS = ('rgb_u8_planar', 'rgb_f32', 'rgb_bf16_planar', 'u16', 'f32')
for _kind in _SHAPE_KINDS:
    _add('up-' + _kind, 'shapes', _kind, (3, 1030), (2, 300), 'up-sampling over three segments: floor(f) < 0 at 0, the clamp at s - 1, spans of ~150 columns')
    _add('sw1-' + _kind, 'shapes', _kind, (2, 600), (3, 1), 'a source row of one pixel: xa = xb = 0 in both segments')
    _add('sw2-' + _kind, 'shapes', _kind, (2, 600), (3, 2), 'a source row of two pixels: every x0 / x1 is 0 or 1')
    _add('sh1-' + _kind, 'shapes', _kind, (3, 530), (1, 700), 'a source of one row: both source rows of every output row are row 0')
    _add('h1-' + _kind, 'shapes', _kind, (1, 515), (1, 1030), 'H = 1 from sH = 1: equal heights, yet no identity')
    _add('aniso-' + _kind, 'shapes', _kind, (7, 700), (3, 1900), 'rows up, columns down: 7 x 700 <- 3 x 1900')
    _add('ident-' + _kind, 'shapes', _kind, (2, 1025), (2, 1025), 'the identity over three segments: one sample per output, no weights')

# residues: an input that does not start on a 16-byte boundary (the byte-by-byte front window of resize_stage), and odd H * W
# (frames 0 / 1 / 2 alternate the output's store shapes); 3 x 515 <- 5 x 1031
for _kind in KINDS:
    _k = KINDS[_kind]
    for _off in ((1, 15) if _k.el == 1 else (_k.el,)):
        _add('res%d-%s' % (_off, _kind), 'residues', _kind, (3, 515), (5, 1031), 'the buffer starts %d bytes past a 16-byte boundary; H W odd' % _off, _off)


# ---- content and reference ------------------------------------------------------------------------------------------------------------
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def _float_bits(rng, shape, half):
    """Seeded noise in [0, 1] as the bit patterns of float32 / float16 / bfloat16, holding 0, 1 and a stripe each of subnormals, the
    smallest normals, -0.0 and the type's largest finite value.  No NaN, no infinity."""
    u = rng.uniform(0, 1, shape).astype(np.float32)
    if half == 'f16':
        bits = u.astype(np.float16).view(np.uint16)
        sub, norm, neg0, big = rng.randint(1, 0x400, shape), 0x0400 + rng.randint(0, 3, shape), 0x8000, 0x7bff
    elif half == 'bf16':
        bits = (u.view(np.uint32) >> 16).astype(np.uint16)
        sub, norm, neg0, big = rng.randint(1, 0x80, shape), 0x0080 + rng.randint(0, 3, shape), 0x8000, 0x7f7f
    else:
        bits = u.view(np.uint32).copy()
        sub, norm, neg0, big = rng.randint(1, 0x800000, shape), 0x00800000 + rng.randint(0, 3, shape), 0x80000000, 0x7f7fffff
    flat = bits.reshape(N, -1)
    idx = np.arange(flat.shape[1]) % 53
    for stripe, v in ((3, sub), (7, norm), (11, neg0), (17, big), (23, 0)):
        m = idx == stripe
        flat[:, m] = np.broadcast_to(np.asarray(v, np.int64), shape).reshape(N, -1)[:, m].astype(bits.dtype)
    return bits


def _widen(bits, half):
    """The float64 value of every bit pattern."""
    if half == 'f16':
        return bits.view(np.float16).astype(np.float64)
    if half == 'bf16':
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float32).astype(np.float64)


def case_input(name):
    """(the array handed to the stage, its float64 values as resize_linear takes them: [N, sH, sW, 3] B G R / [N, sH, sW] metres)."""
    if ('in', name) not in _cache:
        c = CASES[name]
        k = KINDS[c.kind]
        rng = np.random.RandomState(zlib_seed(name))
        if not k.image:
            if c.kind == 'u16':
                arr = rng.randint(0, 65536, (N, c.sH, c.sW)).astype(np.uint16)
                arr[:, 0, 0], arr[:, -1, -1] = 0, 65535
                arr.reshape(N, -1)[:, (np.arange(c.sH * c.sW) % 53) == 5] = 65535
                values = (arr.astype(np.float32) / np.float32(256.0)).astype(np.float64)      # the loader's metres
            else:
                bits = _float_bits(rng, (N, c.sH, c.sW), None)
                plain = np.arange(c.sH * c.sW) % 2 == 0                                       # every other sample a plain distance
                bits.reshape(N, -1)[:, plain] = rng.uniform(0.5, 300.0, (N, int(plain.sum()))).astype(np.float32).view(np.uint32)
                arr, values = bits.view(np.float32), _widen(bits, None)
        else:
            shape = (N, 3, c.sH, c.sW) if k.planar else (N, c.sH, c.sW, 3)
            if k.el == 1:
                arr = rng.randint(0, 256, shape).astype(np.uint8)
                flat = arr.reshape(N, -1)
                flat[:, 0], flat[:, -1] = 0, 255
                flat[:, (np.arange(flat.shape[1]) % 53) == 5] = 255
                flat[:, (np.arange(flat.shape[1]) % 53) == 9] = 0
                values = arr / 255.0
            else:
                bits = _float_bits(rng, shape, k.half)
                arr = bits.view(np.float32) if k.half is None else bits
                values = _widen(bits, k.half)
            if k.planar:
                values = values.transpose(0, 2, 3, 1)
            if k.rgb:
                values = values[..., ::-1]
            values = np.ascontiguousarray(values)
        _cache[('in', name)] = (_frozen(arr), _frozen(values))
    return _cache[('in', name)]


def zlib_seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7fffffff


def case_want(name):
    """[N, H, W, 3] float64 B G R, or [N, H, W] float32 (resize_linear in float64, rounded once): computed once, never written to."""
    if ('want', name) not in _cache:
        c = CASES[name]
        values = case_input(name)[1]
        with np.errstate(over='ignore', under='ignore'):
            want = np.stack([imgops.resize_linear(f, c.W, c.H) for f in values])
            if not KINDS[c.kind].image:
                want = want.astype(np.float32)
        _cache[('want', name)] = _frozen(want)
    return _cache[('want', name)]


def bits_of(a):
    """The array as integers of its bit patterns, so that -0.0 differs from 0.0."""
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def mismatches(got, want):
    return np.argwhere(bits_of(np.ascontiguousarray(got)) != bits_of(np.ascontiguousarray(want)))[:4].tolist()
