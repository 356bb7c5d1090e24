"""Baseline JPEG input frames: the catalogue of files and a numpy statement of the decoding process, shared by
tests/test_jpeg_host.py (the statement on trial against PIL; the host reader and the g++ build of csrc/rr_jpeg.h against the
statement) and tests/test_gpu_jpeg_in.py (the device against the statement).

The statement: ITU-T T.81's baseline process with libjpeg's arithmetic -- jidctint.c's "islow" inverse DCT, jdsample.c's upsampling
(the triangle filters h2v1 / h2v2 where the downsampled width exceeds 2, sample replication at a width of 1 or 2: libjpeg's own
choice of method) and jdcolor.c's fixed-point YCbCr -> RGB.  Sums and products are two's-complement 32-bit and WRAP (numpy int32
arrays), as csrc/rr_jpeg.h states them on uint32_t, so the two agree on any coefficients; agreement with PIL is claimed for the
catalogue's files only.  Files are made by PIL's encoder when a test asks for them; nothing binary is committed."""
import functools
import io

import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
      57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
S444, S422, S420, GREY = 0, 1, 2, 3                       # RR_JPEG_* (PIL's `subsampling` codes, and one for a grey file)
NAMES = {S444: '444', S422: '422', S420: '420', GREY: 'grey'}

# ---- the catalogue -----------------------------------------------------------------------------------------------------------------
SIZES = [(37, 29), (16, 16), (3, 1), (9, 1), (33, 40)]    # W x H, each in 4:4:4, 4:2:2 and 4:2:0
QUALITIES = (50, 92, 100)


def source_image(W, H, seed=1):
    """A smooth image plus noise (R G B bytes)."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([127 + 90 * np.sin(xx / 5. + yy / 7.), xx * 255 / max(W - 1, 1), yy * 255 / max(H - 1, 1)], -1) + rng.normal(0, 25, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(rgb, quality=92, sampling=S420, optimize=False, progressive=False, **kw):
    """PIL's encoder on R G B bytes (or on a 2-D grey array): the file's bytes."""
    from PIL import Image
    f = io.BytesIO()
    if rgb.ndim == 2:
        Image.fromarray(rgb).save(f, 'JPEG', quality=quality, optimize=optimize, progressive=progressive, **kw)
    else:
        Image.fromarray(rgb).save(f, 'JPEG', quality=quality, subsampling=sampling, optimize=optimize, progressive=progressive, **kw)
    return f.getvalue()


@functools.lru_cache(maxsize=None)
def catalogue():
    """[(name, W, H, sampling, bytes)]: every kind of file the reader accepts."""
    out = []
    for (W, H) in SIZES:
        for ss in (S444, S422, S420):
            for q in QUALITIES:
                for opt in (False, True):
                    out.append(('%dx%d_%s_q%d%s' % (W, H, NAMES[ss], q, '_opt' if opt else ''), W, H, ss, encode(source_image(W, H), q, ss, opt)))
    for q in QUALITIES:
        for opt in (False, True):
            out.append(('1x9_444_q%d%s' % (q, '_opt' if opt else ''), 1, 9, S444, encode(source_image(1, 9), q, S444, opt)))
            out.append(('17x9_grey_q%d%s' % (q, '_opt' if opt else ''), 17, 9, GREY, encode(source_image(17, 9)[..., 0].copy(), q, optimize=opt)))
            out.append(('37x29_420_rst1_q%d%s' % (q, '_opt' if opt else ''), 37, 29, S420,
                        encode(source_image(37, 29), q, S420, opt, restart_marker_blocks=1)))
            out.append(('37x29_420_rstrow_q%d%s' % (q, '_opt' if opt else ''), 37, 29, S420,
                        encode(source_image(37, 29), q, S420, opt, restart_marker_rows=1)))
    return out


def kinds():
    """One file per (size, sampling, restart) kind of the catalogue -- quality 92, standard tables: what the GPU tier runs."""
    return [c for c in catalogue() if c[0].endswith('_q92')]


# ---- the numpy statement -----------------------------------------------------------------------------------------------------------
class Refused(Exception):
    pass


def parse(b):
    """Markers up to the scan: (H, W, components, tables, Huffman tables, restart interval, offset of the entropy-coded data)."""
    if b[:2] != b'\xff\xd8':
        raise Refused('no SOI')
    p, q, ht, comps, dri = 2, {}, {}, None, 0
    while True:
        if b[p] != 0xFF:
            raise Refused('marker expected')
        while b[p] == 0xFF:
            p += 1
        m = b[p]
        p += 1
        L = (b[p] << 8) | b[p + 1]
        seg = b[p + 2:p + L]
        p += L
        if m == 0xDB:
            s = 0
            while s < len(seg):
                pq, tq = seg[s] >> 4, seg[s] & 15
                if pq != 0:
                    raise Refused('16-bit table')
                t = np.zeros(64, np.int64)
                for k in range(64):
                    t[ZZ[k]] = seg[s + 1 + k]
                q[tq] = t
                s += 65
        elif m == 0xC0:
            if seg[0] != 8:
                raise Refused('precision')
            H, W, n = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            comps = [dict(id=seg[6 + 3 * i], h=seg[7 + 3 * i] >> 4, v=seg[7 + 3 * i] & 15, tq=seg[8 + 3 * i]) for i in range(n)]
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Refused('not baseline')
        elif m == 0xC4:
            s = 0
            while s < len(seg):
                tc, th = seg[s] >> 4, seg[s] & 15
                cnt = list(seg[s + 1:s + 17])
                s += 17
                code, tab = 0, {}
                for ln in range(16):
                    for _ in range(cnt[ln]):
                        tab[(ln + 1, code)] = seg[s]
                        s += 1
                        code += 1
                    code <<= 1
                ht[(tc, th)] = tab
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if seg[0] != len(comps):
                raise Refused('several scans')
            for i, c in enumerate(comps):
                assert seg[1 + 2 * i] == c['id']
                c['td'], c['ta'] = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
            return H, W, comps, q, ht, dri, p


class Bits:
    """The entropy-coded segment's bits, MSB first: FF 00 un-stuffed; the reader stands still at any other marker."""

    def __init__(self, b, p):
        self.b, self.p, self.cur, self.n = b, p, 0, 0

    def bit(self):
        if self.n == 0:
            c = self.b[self.p]
            if c == 0xFF:
                if self.b[self.p + 1] != 0:
                    raise Refused('data ends at a marker')
                self.p += 2
            else:
                self.p += 1
            self.cur, self.n = c, 8
        self.n -= 1
        return (self.cur >> self.n) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def huff(self, tab):
        c = 0
        for ln in range(1, 17):
            c = (c << 1) | self.bit()
            if (ln, c) in tab:
                return tab[(ln, c)]
        raise Refused('code not in table')

    def restart(self, k):
        self.n = 0
        assert self.b[self.p] == 0xFF and self.b[self.p + 1] == 0xD0 + (k & 7), 'RST%d expected' % (k & 7)
        self.p += 2


def _extend(v, n):
    return v if n == 0 or v >= (1 << (n - 1)) else v - (1 << n) + 1


def geometry(W, H, sampling):
    """MCUs across / down and the padded planes [(rows, columns)] of a frame: Y, then Cb and Cr."""
    hs, vs = (2 if sampling in (S422, S420) else 1), (2 if sampling == S420 else 1)
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
    planes = [(mh * vs * 8, mw * hs * 8)] + ([] if sampling == GREY else [(mh * 8, mw * 8)] * 2)
    return hs, vs, mw, mh, planes


def sampling_of(comps):
    f = [(c['h'], c['v']) for c in comps]
    if len(f) == 1:
        return GREY
    if len(f) == 3 and f[1:] == [(1, 1), (1, 1)] and f[0] in ((1, 1), (2, 1), (2, 2)):
        return {(1, 1): S444, (2, 1): S422, (2, 2): S420}[f[0]]
    raise Refused('sampling')


def coefficients(b):
    """The file's coefficient record as the library lays it out: (W, H, sampling, tables [ncomp, 64] in natural order, coefficients
    [blocks, 64] int16 in natural order -- per component in raster order over its padded plane, Y then Cb then Cr)."""
    H, W, comps, q, ht, dri, p = parse(b)
    sampling = sampling_of(comps)
    hs, vs, mw, mh, planes = geometry(W, H, sampling)
    if hs == 2 and W < 3:
        raise Refused('subsampled chroma in a frame narrower than 3')
    blocks = [np.zeros((ph // 8, pw // 8, 64), np.int64) for (ph, pw) in planes]
    br = Bits(b, p)
    pred = [0] * len(comps)
    for mi in range(mw * mh):
        if dri and mi and mi % dri == 0:
            br.restart(mi // dri - 1)
            pred = [0] * len(comps)
        my, mx = divmod(mi, mw)
        for ci, c in enumerate(comps):
            ch, cv = (hs, vs) if ci == 0 else (1, 1)
            for by in range(cv):
                for bx in range(ch):
                    co = blocks[ci][my * cv + by, mx * ch + bx]
                    t = br.huff(ht[(0, c['td'])])
                    pred[ci] += _extend(br.bits(t), t)
                    co[0] = pred[ci]
                    k = 1
                    while k < 64:
                        rs = br.huff(ht[(1, c['ta'])])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r == 15:
                                k += 16
                                continue
                            break
                        k += r
                        co[ZZ[k]] = _extend(br.bits(s), s)
                        k += 1
    assert b[br.p:br.p + 2] == b'\xff\xd9', 'EOI expected behind the scan'
    tables = np.stack([q[c['tq']] for c in comps]).astype(np.uint16)
    return W, H, sampling, tables, np.concatenate([bl.reshape(-1, 64) for bl in blocks]).astype(np.int16)


def _pass(i):
    """One 1-D pass of jidctint.c on int32 arrays i[0..7] (wrapping): the eight sums before descaling."""
    c = lambda v: np.int32(v)
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * c(4433)
    t2, t3 = z1 - z3 * c(15137), z1 + z2 * c(6270)
    t0, t1 = (i[0] + i[4]) << c(13), (i[0] - i[4]) << c(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * c(9633)
    a0, a1, a2, a3 = a0 * c(2446), a1 * c(16819), a2 * c(25172), a3 * c(12299)
    z1, z2, z3, z4 = -(z1 * c(7373)), -(z2 * c(20995)), -(z3 * c(16069)) + z5, -(z4 * c(3196)) + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]


def idct_blocks(coef, table):
    """[n, 64] int16 coefficients (natural order) times the [64] table -> [n, 8, 8] uint8 samples.  32-bit, wrapping."""
    with np.errstate(over='ignore'):
        x = (coef.astype(np.int32) * table.astype(np.int64).astype(np.int32)[None, :]).reshape(-1, 8, 8)
        cols = _pass([x[:, y, :] for y in range(8)])                                  # down the columns: cols[y][n, x]
        ws = np.stack([(o + np.int32(1 << 10)) >> np.int32(11) for o in cols], 1)   # [n, y, x]
        rows = _pass([ws[:, :, xx] for xx in range(8)])                               # along the rows: rows[x][n, y]
        out = np.stack([((o + np.int32(1 << 17)) >> np.int32(18)) + np.int32(128) for o in rows], 2)
    return np.clip(out, 0, 255).astype(np.uint8)


def up_h2v1(pl, dh, dw):
    r = pl[:dh, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(r, 2, 1)
    o = np.zeros((dh, 2 * dw), np.int64)
    o[:, 0] = r[:, 0]
    o[:, 2::2] = (3 * r[:, 1:] + r[:, :-1] + 1) >> 2
    o[:, 1:-1:2] = (3 * r[:, :-1] + r[:, 1:] + 2) >> 2
    o[:, -1] = r[:, -1]
    return o


def up_h2v2(pl, dh, dw):
    r = pl[:dh, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(np.repeat(r, 2, 0), 2, 1)
    o = np.zeros((2 * dh, 2 * dw), np.int64)
    for v in (0, 1):
        near = np.clip(np.arange(dh) + (1 if v else -1), 0, dh - 1)
        s = 3 * r + r[near]
        o[v::2, 0] = (4 * s[:, 0] + 8) >> 4
        o[v::2, 2::2] = (3 * s[:, 1:] + s[:, :-1] + 8) >> 4
        o[v::2, 1:-1:2] = (3 * s[:, :-1] + s[:, 1:] + 7) >> 4
        o[v::2, -1] = (4 * s[:, -1] + 7) >> 4
    return o


def ycc_bgr(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def planes_of(W, H, sampling, tables, coef):
    """The component planes of bytes at their padded sizes."""
    out, at = [], 0
    for ci, (ph, pw) in enumerate(geometry(W, H, sampling)[4]):
        n = (ph // 8) * (pw // 8)
        px = idct_blocks(coef[at:at + n], tables[ci])
        out.append(px.reshape(ph // 8, pw // 8, 8, 8).transpose(0, 2, 1, 3).reshape(ph, pw))
        at += n
    return out


def pixels_of(W, H, sampling, tables, coef):
    """The frame, B G R bytes [H, W, 3], of a coefficient record."""
    hs, vs = geometry(W, H, sampling)[:2]
    pl = planes_of(W, H, sampling, tables, coef)
    y = pl[0][:H, :W]
    if sampling == GREY:
        return np.stack([y] * 3, -1).astype(np.uint8)
    dh, dw = -(-H // vs), -(-W // hs)
    up = {S444: lambda p: p, S422: lambda p: up_h2v1(p, dh, dw), S420: lambda p: up_h2v2(p, dh, dw)}[sampling]
    return ycc_bgr(y, up(pl[1])[:H, :W], up(pl[2])[:H, :W])


def decode_bgr(b):
    return pixels_of(*coefficients(b))


def pil_bgr(b):
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(io.BytesIO(b)).convert('RGB'))[..., ::-1])


def record_of(W, H, sampling, tables, coef):
    """The record's bytes as rr_jpeg_read_record lays them out (rr_jpeg_header, 416 bytes, then the coefficients)."""
    hdr = np.zeros(416, np.uint8)
    hdr[:32].view(np.int32)[:5] = [0x314a5252, W, H, sampling, len(tables)]
    hdr[32:32 + 128 * len(tables)].view(np.uint16)[:] = tables.reshape(-1)
    return np.concatenate([hdr, np.ascontiguousarray(coef).view(np.uint8).reshape(-1)])
