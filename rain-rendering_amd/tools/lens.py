"""Drops on the lens: adherent raindrops on the camera's lens or windshield.  numpy only.

Two things live here, both the host STATEMENT of what the device does (csrc/rr_lens.h, k_lens_drops):

  * `LensDrops`: where the drops are.  Counter-based like the particle field (tools/particles.py): slot j has a life period and a
    phase for good, a life's own Philox block draws the drop, a drop neither moves nor changes during a life, and `.table(k)` is a
    pure function of (seed, k).
  * `apply_numpy`: the pixel arithmetic.  Every drop is a small inverted, minified, defocused view of the INPUT image with a soft
    edge and a dark rim.  + - * / sqrt floor rint min max only, in the order written here; coordinates in float64, pixel values
    in float32.

A drop record (LENS_DROP_DTYPE, rr_lens_drop: 32 bytes, all float32): cx, cy centre in pixels; rx, ry semi-axes in pixels; mag >= 1
how many times wider the field seen through the drop is; edge in (0, 1] the soft edge's width; rim in [0, 1] the rim darkening;
sigma_class the index of the drop's blur class (a float holding a small integer).  The blur table of a call is
(class_radius int32[n_classes], weights float32[16, 31]): class c has radius R = class_radius[c] <= 15 and the 2 R + 1 taps
weights[c, :2 R + 1]."""
import numbers

import numpy as np

from .particles import _key, _life_counter, philox4x32, unit32

RR_MAX_LENS_DROPS = 128
MAX_CLASSES = 16
MAX_RADIUS = 15
TAPS = 2 * MAX_RADIUS + 1

LENS_DROP_DTYPE = np.dtype([('cx', '<f4'), ('cy', '<f4'), ('rx', '<f4'), ('ry', '<f4'), ('mag', '<f4'), ('edge', '<f4'), ('rim', '<f4'),
                            ('sigma_class', '<f4')])
assert LENS_DROP_DTYPE.itemsize == 32


# ---- the blur table ------------------------------------------------------------------------------------------------
def gaussian_class(sigma):
    """(R, the 2 R + 1 taps as float32) of a truncated, normalised Gaussian: R = min(ceil(3 sigma), 15); sigma 0 is the single tap 1."""
    sigma = float(sigma)
    R = int(min(np.ceil(3.0 * sigma), MAX_RADIUS)) if sigma > 0 else 0
    if R == 0:
        return 0, np.ones(1, np.float32)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / sigma) ** 2)
    return R, (w / w.sum()).astype(np.float32)


def blur_table(sigmas):
    """The blur table of up to 16 classes of these standard deviations (pixels): (class_radius int32[n], weights float32[16, 31])."""
    sigmas = [float(s) for s in np.atleast_1d(sigmas)]
    if not 1 <= len(sigmas) <= MAX_CLASSES or any(not np.isfinite(s) or s < 0 for s in sigmas):
        raise ValueError("blur classes %r: expected 1 to %d finite standard deviations >= 0" % (sigmas, MAX_CLASSES))
    radius = np.zeros(len(sigmas), np.int32)
    weights = np.zeros((MAX_CLASSES, TAPS), np.float32)
    for c, s in enumerate(sigmas):
        radius[c], w = gaussian_class(s)
        weights[c, :len(w)] = w
    return radius, weights


def check_weights(weights):
    """(class_radius, weights) as the contiguous arrays a call hands over; ValueError for a table outside the limits."""
    try:
        radius, w = weights
    except (TypeError, ValueError):
        raise ValueError("the blur table is (class_radius, weights)")
    radius = np.ascontiguousarray(radius, np.int32).reshape(-1)
    w = np.ascontiguousarray(w, np.float32)
    if not 1 <= len(radius) <= MAX_CLASSES or w.shape != (MAX_CLASSES, TAPS) or radius.min() < 0 or radius.max() > MAX_RADIUS:
        raise ValueError("the blur table holds 1 to %d classes of radius 0 .. %d and float32 weights [%d, %d]" %
                         (MAX_CLASSES, MAX_RADIUS, MAX_CLASSES, TAPS))
    if not np.isfinite(w).all():
        raise ValueError("the blur table's weights must be finite")
    return radius, w


# ---- where a drop is -----------------------------------------------------------------------------------------------
def drop_box(d, H, W):
    """The drop's bounding box clipped to the frame, inclusive: (x0, x1, y0, y1), or None when nothing of it is inside.
    floor(c - r) .. floor(c + r) + 1 in float64 on the record's float32 values (rr_lens.h lens_box)."""
    cx, cy, rx, ry = (np.float64(d[k]) for k in ('cx', 'cy', 'rx', 'ry'))
    x0, x1 = max(np.floor(cx - rx), 0.0), min(np.floor(cx + rx) + 1.0, float(W - 1))
    y0, y1 = max(np.floor(cy - ry), 0.0), min(np.floor(cy + ry) + 1.0, float(H - 1))
    if not (x1 >= x0 and y1 >= y0):
        return None
    return int(x0), int(x1), int(y0), int(y1)


def drop_boxes(t, H, W):
    """drop_box of every record of a table at once: (x0, x1, y0, y1 float64 arrays, inside bool array)."""
    cx, cy, rx, ry = (t[k].astype(np.float64) for k in ('cx', 'cy', 'rx', 'ry'))
    x0, x1 = np.maximum(np.floor(cx - rx), 0.0), np.minimum(np.floor(cx + rx) + 1.0, float(W - 1))
    y0, y1 = np.maximum(np.floor(cy - ry), 0.0), np.minimum(np.floor(cy + ry) + 1.0, float(H - 1))
    return x0, x1, y0, y1, (x1 >= x0) & (y1 >= y0)


def boxes_overlap(a, b):
    return a[0] <= b[1] and b[0] <= a[1] and a[2] <= b[3] and b[2] <= a[3]


def check_table(table, H, W, n_classes):
    """ValueError for a table the library refuses (rr_lens_drops_device's RR_E_ARG list): the count, a field that is not finite or
    out of range, a bad class, two overlapping bounding boxes."""
    t = np.asarray(table)
    if t.dtype != LENS_DROP_DTYPE or t.ndim != 1:
        raise ValueError("a drop table is a 1-d array of LENS_DROP_DTYPE records")
    if len(t) > RR_MAX_LENS_DROPS:
        raise ValueError("%d drops in a frame: at most %d" % (len(t), RR_MAX_LENS_DROPS))
    for k in LENS_DROP_DTYPE.names:
        if not np.isfinite(t[k]).all():
            raise ValueError("lens drop field %s is not finite" % k)
    if len(t) == 0:
        return
    cls = t['sigma_class']
    if (t['rx'] <= 0).any() or (t['ry'] <= 0).any() or (t['mag'] < 1).any() or (t['edge'] <= 0).any() or (t['edge'] > 1).any() or \
            (t['rim'] < 0).any() or (t['rim'] > 1).any() or (cls != np.floor(cls)).any() or (cls < 0).any() or (cls >= n_classes).any():
        raise ValueError("lens drop out of range: rx, ry > 0, mag >= 1, edge in (0, 1], rim in [0, 1], class in 0 .. %d" % (n_classes - 1))
    boxes = [b for b in (drop_box(d, H, W) for d in t) if b is not None]
    for i in range(len(boxes)):
        for j in range(i):
            if boxes_overlap(boxes[i], boxes[j]):
                raise ValueError("the bounding boxes of two lens drops of one frame overlap: %r and %r" % (boxes[j], boxes[i]))


# ---- the pixel arithmetic ------------------------------------------------------------------------------------------
def _rho2(d, qx, qy):
    """(dx [w], dy [h], rho^2 [h, w]) at the integer pixel coordinates qx, qy: float64."""
    dx = qx.astype(np.float64) - np.float64(d['cx'])
    dy = qy.astype(np.float64) - np.float64(d['cy'])
    u, v = dx / np.float64(d['rx']), dy / np.float64(d['ry'])
    return dx, dy, (u * u)[None, :] + (v * v)[:, None]


def _sample_axis(c, mag, dq, g, size):
    """Clamped sample coordinate along one axis -> (lower index, upper index, float32 fraction)."""
    s = c - (mag * dq) * g
    s = np.minimum(np.maximum(s, 0.0), float(size - 1))
    i0 = np.floor(s)
    f = (s - i0).astype(np.float32)
    i0 = i0.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), f


def refract(img, d, qx, qy):
    """V(q) [3, h, w] float32: the input image `img` ([3, H, W], any dtype; values enter as float32) seen through drop d at the pixels
    (qx, qy), upside down and mirrored, bilinear."""
    _, H, W = img.shape
    dx, dy, r2 = _rho2(d, qx, qy)
    g = 1.0 / np.sqrt(1.0 - 0.75 * np.minimum(r2, 1.0))
    mag = np.float64(d['mag'])
    x0, x1, fx = _sample_axis(np.float64(d['cx']), mag, dx[None, :], g, W)
    y0, y1, fy = _sample_axis(np.float64(d['cy']), mag, dy[:, None], g, H)
    p00, p01 = img[:, y0, x0].astype(np.float32), img[:, y0, x1].astype(np.float32)
    p10, p11 = img[:, y1, x0].astype(np.float32), img[:, y1, x1].astype(np.float32)
    top = p00 + fx * (p01 - p00)
    bot = p10 + fx * (p11 - p10)
    return top + fy * (bot - top)


def blur_pass(v, w, axis):
    """One pass of the separable blur along `axis` of v (float32): taps added in ascending offset order; the output is 2 R shorter."""
    n = v.shape[axis] - (len(w) - 1)
    acc = None
    for k in range(len(w)):
        term = np.float32(w[k]) * np.take(v, np.arange(k, k + n), axis=axis)
        acc = term if acc is None else acc + term
    return acc


def coverage(r2, edge):
    """A = t t (3 - 2 t), t = clamp((1 - rho^2) / edge, 0, 1): float64 in, float32 out."""
    t = np.minimum(np.maximum((1.0 - r2) / np.float64(edge), 0.0), 1.0)
    return (t * t * (3.0 - 2.0 * t)).astype(np.float32)


def apply_drop(img, out, alpha, d, radius, weights):
    """Drop d of one frame: reads `img` [3, H, W], writes its box of `out` (same dtype) and of `alpha` ([H, W] float32 or None)."""
    _, H, W = img.shape
    box = drop_box(d, H, W)
    if box is None:
        return
    x0, x1, y0, y1 = box
    c = int(d['sigma_class'])
    R = int(radius[c])
    w = weights[c, :2 * R + 1]
    qx, qy = np.arange(x0, x1 + 1), np.arange(y0, y1 + 1)
    hx = np.clip(np.arange(x0 - R, x1 + R + 1), 0, W - 1)      # the halo is evaluated at q clamped to the frame
    hy = np.clip(np.arange(y0 - R, y1 + R + 1), 0, H - 1)
    B = blur_pass(blur_pass(refract(img, d, hx, hy), w, 2), w, 1)
    _, _, r2 = _rho2(d, qx, qy)
    A = coverage(r2, d['edge'])
    rimf = (1.0 - (np.float64(d['rim']) * r2) * r2).astype(np.float32)
    inp = img[:, y0:y1 + 1, x0:x1 + 1].astype(np.float32)
    res = (np.float32(1.0) - A) * inp + A * (rimf * B)
    if img.dtype == np.uint8:
        res = np.minimum(np.maximum(np.rint(res), np.float32(0.0)), np.float32(255.0)).astype(np.uint8)
    sub = out[:, y0:y1 + 1, x0:x1 + 1]
    sub[...] = np.where(A == 0, sub, res)                       # A == 0: the input value, bit for bit
    if alpha is not None:
        alpha[y0:y1 + 1, x0:x1 + 1] = A


def apply_numpy(images, tables, weights, alpha=False):
    """The statement of the lens pass: `images` planar [n, 3, H, W] uint8 or float32, `tables` n drop tables (LENS_DROP_DTYPE arrays),
    `weights` the blur table.  Returns the images with the drops on them (same dtype), and with alpha=True also [n, H, W] float32:
    A inside the drops, 0 elsewhere.  Every drop refracts the INPUT image; the boxes of one frame are disjoint (ValueError)."""
    images = np.asarray(images)
    if images.ndim != 4 or images.shape[1] != 3 or images.dtype not in (np.uint8, np.float32):
        raise ValueError("images must be [n, 3, H, W] uint8 or float32")
    n, _, H, W = images.shape
    if len(tables) != n:
        raise ValueError("%d drop tables for %d images" % (len(tables), n))
    radius, w = check_weights(weights)
    out = images.copy()
    al = np.zeros((n, H, W), np.float32) if alpha else None
    for f in range(n):
        check_table(tables[f], H, W, len(radius))
        for d in tables[f]:
            apply_drop(images[f], out[f], None if al is None else al[f], d, radius, w)
    return (out, al) if alpha else out


def alpha_label(alpha):
    """The byte label the frame pipeline writes for a coverage A (rr_pipeline_lens.alpha_png; rr_lens.h lens_label):
    v = clamp(rint(float32(A) * float32(255)), 0, 255), one float32 multiply, then half to even.  uint8, the shape of `alpha`."""
    a = np.asarray(alpha, np.float32)
    return np.minimum(np.maximum(np.rint(a * np.float32(255.0)), np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


# ---- the generator -------------------------------------------------------------------------------------------------
def _range(name, v, lo=None, hi=None, lo_open=False):
    try:
        a, b = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError("%s %r: expected a (low, high) pair of numbers" % (name, v))
    bad = not (np.isfinite(a) and np.isfinite(b)) or a > b
    bad = bad or (lo is not None and (a <= lo if lo_open else a < lo)) or (hi is not None and b > hi)
    if bad:
        raise ValueError("%s %r: expected low <= high within %s%s, %s]" % (name, v, '(' if lo_open else '[', lo, 'inf' if hi is None else hi))
    return a, b


class LensDrops:
    """Adherent drops for H x W frames: `count` slots, each always holding one drop that sits still for a life of life_s seconds and
    is then replaced by a new one elsewhere.  `.table(k)` are the drops shown at frame k (time k / hz): those whose bounding box no
    OLDER live drop overlaps, so a drop that is shown stays shown until it dies."""

    def __init__(self, H, W, count=40, radius=(2, 40), aspect=(1.0, 1.4), mag=(3, 8), blur=(0.5, 4.0), edge=(0.1, 0.4), rim=(0.2, 0.6),
                 life_s=(2, 20), hz=10, seed=0):
        for name, v in (('H', H), ('W', W), ('count', count)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < (0 if name == 'count' else 1):
                raise ValueError("%s %r: expected a positive integer" % (name, v))
        if count > RR_MAX_LENS_DROPS:
            raise ValueError("count %d: at most %d drops on a lens" % (count, RR_MAX_LENS_DROPS))
        self.H, self.W, self.count = int(H), int(W), int(count)
        self.radius = _range('radius', radius, 0.0, lo_open=True)
        self.aspect = _range('aspect', aspect, 1.0)
        self.mag = _range('mag', mag, 1.0)
        self.blur = _range('blur', blur, 0.0)
        self.edge = _range('edge', edge, 0.0, 1.0, lo_open=True)
        self.rim = _range('rim', rim, 0.0, 1.0)
        self.life_s = _range('life_s', life_s, 0.0, lo_open=True)
        if isinstance(hz, bool) or not isinstance(hz, numbers.Number) or not np.isfinite(hz) or hz <= 0:
            raise ValueError("hz %r: expected frames per second > 0" % (hz,))
        self.hz = float(hz)
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral):
            raise ValueError("seed %r: expected an integer" % (seed,))
        self.seed = int(seed)
        # the instance's blur classes: the range cut into at most 16 standard deviations
        lo, hi = self.blur
        self.sigmas = [lo] if lo == hi else list(np.linspace(lo, hi, MAX_CLASSES))
        self._weights = blur_table(self.sigmas)
        # slot j for good: life period and phase, Philox block (j, 0, 0, 1)
        j = np.arange(self.count, dtype=np.uint64)
        a = philox4x32(j, 0, 0, 1, *_key(self.seed))
        self._T = self.life_s[0] + unit32(a[0]) * (self.life_s[1] - self.life_s[0])
        self._phase = unit32(a[1])

    def _args(self):
        return dict(count=self.count, radius=self.radius, aspect=self.aspect, mag=self.mag, blur=self.blur, edge=self.edge, rim=self.rim,
                    life_s=self.life_s, hz=self.hz)

    _SPEC_KEYS = ('count', 'radius', 'aspect', 'mag', 'blur', 'edge', 'rim', 'life_s', 'hz', 'seed')

    @classmethod
    def from_spec(cls, spec, H, W, hz):
        """The drops of a command line (main.py --lens_drops): COUNT[,SEED], or the path of a JSON file holding an object of LensDrops
        keywords (count, radius, aspect, mag, blur, edge, rim, life_s, hz, seed).  H, W and -- unless the file names one -- hz come
        from the caller."""
        import json
        import os
        spec = str(spec).strip()
        parts = spec.split(',')
        if 1 <= len(parts) <= 2 and all(p.strip().lstrip('+-').isdigit() for p in parts):
            return cls(H, W, count=int(parts[0]), seed=int(parts[1]) if len(parts) > 1 else 0, hz=hz)
        if not os.path.isfile(spec):
            raise ValueError("lens drops %r: expected COUNT[,SEED] or the path of a JSON file of LensDrops keywords" % (spec,))
        try:
            with open(spec) as f:
                kw = json.load(f)
        except (OSError, ValueError) as e:
            raise ValueError("lens drops %r: expected a JSON file of LensDrops keywords (%s)" % (spec, e))
        if not isinstance(kw, dict) or any(k not in cls._SPEC_KEYS for k in kw):
            raise ValueError("lens drops %r: expected a JSON object with keys among %s" % (spec, ', '.join(cls._SPEC_KEYS)))
        kw.setdefault('hz', hz)
        return cls(H, W, **kw)

    def weights(self):
        """The blur table of every call with this instance's tables."""
        return self._weights

    def for_view(self, v):
        """The drops on the lens of camera v of a rig: the same settings under a seed derived from (seed, v)."""
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
            raise ValueError("view %r: expected an index >= 0" % (v,))
        w = philox4x32(int(v), 0, 0, 0x4C454E53, *_key(self.seed))
        return LensDrops(self.H, self.W, seed=int(w[0]) | (int(w[1]) << 32), **self._args())

    def lives(self, frame_index):
        """(life number, birth time in seconds) of every slot at frame `frame_index`."""
        if isinstance(frame_index, bool) or not isinstance(frame_index, numbers.Integral) or frame_index < 0:
            raise ValueError("frame_index %r: expected an integer >= 0" % (frame_index,))
        t = int(frame_index) / self.hz
        g = np.floor(t / self._T + self._phase)
        return g, (g - self._phase) * self._T

    def slots(self, frame_index):
        """Every slot's live drop at frame `frame_index`, shown or not: (records [count], birth [count], kept [count] bool)."""
        g, born = self.lives(frame_index)
        j = np.arange(self.count, dtype=np.uint64)
        key = _key(self.seed)
        b = [unit32(w) for w in philox4x32(*_life_counter(j, g, 1), *key)]
        c = [unit32(w) for w in philox4x32(*_life_counter(j, g, 2), *key)]
        rec = np.zeros(self.count, LENS_DROP_DTYPE)
        rec['cx'] = b[0] * self.W
        rec['cy'] = b[1] * self.H
        rx = self.radius[0] * (self.radius[1] / self.radius[0]) ** b[2]            # log-uniform
        rec['rx'] = rx
        rec['ry'] = rx * (self.aspect[0] + b[3] * (self.aspect[1] - self.aspect[0]))      # ry >= rx: gravity elongates the drop
        rec['ry'] = np.maximum(rec['ry'], rec['rx'])
        rec['mag'] = np.maximum(self.mag[0] + c[0] * (self.mag[1] - self.mag[0]), 1.0)
        n_cls = len(self.sigmas)
        rec['sigma_class'] = np.minimum(np.floor(c[1] * n_cls), n_cls - 1)
        rec['edge'] = np.minimum(self.edge[0] + c[2] * (self.edge[1] - self.edge[0]), 1.0)
        rec['rim'] = np.minimum(self.rim[0] + c[3] * (self.rim[1] - self.rim[0]), 1.0)
        x0, x1, y0, y1, inside = drop_boxes(rec, self.H, self.W)
        over = (x0[:, None] <= x1[None, :]) & (x0[None, :] <= x1[:, None]) & (y0[:, None] <= y1[None, :]) & (y0[None, :] <= y1[:, None])
        slot = np.arange(self.count)
        older = (born[None, :] < born[:, None]) | ((born[None, :] == born[:, None]) & (slot[None, :] < slot[:, None]))     # [i, o]: o is older than i
        kept = inside & ~(over & older & inside[None, :]).any(axis=1)
        return rec, born, kept

    def table(self, frame_index):
        """The drop records shown at frame `frame_index`, in slot order: a pure function of (seed, frame_index)."""
        rec, _, kept = self.slots(frame_index)
        return np.ascontiguousarray(rec[kept][:RR_MAX_LENS_DROPS])
