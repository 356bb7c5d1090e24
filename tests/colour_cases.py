"""The colour branch's per-drop constants against a float64 reference: a catalogue of environment maps and drop tables aimed at
the places where k_fov_vertices -> k_fov_sort -> k_fov_dda / k_fov_spans -> k_fov_sums32 / k_fov_sums -> k_colour (rainhip.hip)
branch, the reference, and a bound on what the float route may lose, derived from k_fov_sums32's summation order.

Inputs.  The image is 64 x 128 and fixed; the environment map's size is the case's own (rr_frame_in.He / We).  Drops are a
few template records of the product's packer (compositor_cases.Templates) at image positions inside the frame, so every one
has status 0 and a footprint.  A record's field of view follows the mid-point of wps / wpe alone and its tile |wps.z| alone
(rr_device.h fov_setup, plan_drop): a case gives every drop a mid-point of its own -- a direction on the whole sphere, 1.5 to
6 m from the camera -- and keeps |wps.z|.  The map is pseudo-random per texel (x, y in 0.2 .. 0.45, Y log-uniform over two
decades) times a tenfold luminance step between its halves, with the product's solid angles: one texel gained or lost moves
a sum by far more than rounding.  Cones: the product's 165 degrees, and 60 and 12 through make_camera(fov=...).

The reference (reference_sums, reference_K): polygons of the host build's emu_plan (float64, pinned to the reference by the
golden vectors), spans of emu_rowspans under the case's rule, sums from a numpy float64 prefix table, then the float64 chain
of bad_weather.py:397-412 on a gray value of 1.  unmix() takes three constants back to (x, y, Yg), the quantities whose
error follows from the sums directly.

The bound (Map.entry_bound, span_bound, xyY_bound) -- u = 2^-24, every term non-negative, so a sum's relative error is at most
gamma_k = k u / (1 - k u) when no term passes through more than k roundings.  A term of the prefix entry o ("through the
lane's second column", k_fov_sums32's `o[k] = basev[k] + ps[e][k]`) passes through
    its product                       1   (a float64 map: 3 -- both factors are rounded to float as they arrive)
    pa + pb, the pair sum             1
    wave_incl_scan_f32                6   (four row steps, two row broadcasts)
    + carry                        EMAX   (one per pass of 128 columns; the first pass adds an exact zero, counted anyway)
    row16_incl_scan_f32 over s_wt     4
    basev + ps                        1
k = 13 + EMAX for a float map, 15 + EMAX for a float64 one: |dP[j]| <= gamma_k P[j] for an entry through a pair's second
column.  The entry through a pair's FIRST column is o - pb: its error is o's plus one rounding of the difference,
|dP[j]| <= gamma_k P[j + 1] + u P[j] -- not 16 u P[j]: the neighbour may be a hundred times brighter.  (The map's last column
on an odd width has pb = 0: the entry is o.)  A span's difference adds one rounding, a band's running sum at most gamma_rpb
of what it holds (rpb rows; adding an empty row's zero is exact), the bands are added in double:
    |dS| <= (1 + gamma_rpb) sum_rows (B[xr + 1] + B[xl]) (1 + u) + (u + gamma_rpb) S.
The whole-map sums take the row's last entry (an `o`) into doubles: |d sumW| <= sum_rows B[We].  xyY_bound carries these to
x = S0 / S3, y = S1 / S3 and Yg to first order with the second-order term of the quotient kept, plus 1e-12 relative for the
float64 chain itself.  Nothing in it is fitted to a device result.  The float64 routes are held to the suite's 1e-9 max|K|."""
import ctypes
import os
import re

import numpy as np

import helpers as h
from oracle import render as orc


def _hip_source():
    return open(os.path.join(h.ROOT, 'rain-rendering_amd', 'csrc', 'rainhip.hip')).read()


def _hip_constant(name):
    m = re.search(r'constexpr int %s = (\w+);' % name, _hip_source())
    assert m, name
    v = m.group(1)
    if not v.isdigit():                                   # `constexpr int DDA_WAVES = RR_DDA_WAVES;` <- `#define RR_DDA_WAVES 1`
        m = re.search(r'#define %s (\d+)' % v, _hip_source())
        assert m, v
        v = m.group(1)
    return int(v)


COL_PARTS = _hip_constant('COL_PARTS')            # row bands of the map
HE_MAX = _hip_constant('HE_MAX')                  # tallest map of the fast path
FOV_WE_MAX = _hip_constant('FOV_WE_MAX')          # widest map of the fast path
FOV_SORT_WAVES = _hip_constant('FOV_SORT_WAVES')  # k_fov_sort: 64 * FOV_SORT_WAVES drops per sweep
DDA_WAVES = _hip_constant('DDA_WAVES')
# sizes the launch code states as literals; a rewrite that moves one of them moves these lines with it
NT = 1024            # `const int NT = 1024;` threads of a k_fov_sums / k_fov_sums32 workgroup: 16 waves share a map row
PASS_COLS = 128      # `const int cl = e * 128 + 2 * lane`: columns a wave takes per pass, two per lane
E1_WE_MAX = 2048     # `const bool e1 = passes(NT) <= 1;` 16 waves x 128 columns: wider maps take the EMAX = 2 instances
SPANS_H = (384, 512)  # `if (dm.He <= 384)` k_fov_spans<6>, `else if (dm.He <= 512)` <8>, else <16>
TEXELS_MAX = 1 << 22  # fov_fast_path: `(int64_t)dm.We * dm.He < (1 << 22)`
U = 2.0 ** -24

IMG_H, IMG_W = 64, 128
CONES = (165, 60, 12)
GRAY_Y = float(orc.convert_rgb_to_xyY(np.ones(3))[2])      # Y of a gray value of 1


# ---------------------------------------------------------------------------
# what the launch code does with a call (rr_render_frames, "k_fov_sums")
# ---------------------------------------------------------------------------
def predict(He, We, ns, dpt=0, route='f32', env32=True, dda=1, general=False):
    """ns: the drop counts of the call's frames.  route: 'f32' (the default float route), 'f64' (float64 composite or
    RR_OPT_FOV_F32 0)."""
    fast = not general and He <= HE_MAX and We <= FOV_WE_MAX and He * We < TEXELS_MAX
    out = dict(fast=fast, instances=set(), spans=None)
    if not fast:
        out['instances'] = {'k_fov_poly_general', 'k_fov_sums_general'}
        return out
    max_drops = max(ns)
    Cw = ((We + NT // 64 - 1) // (NT // 64) + 1) & ~1
    emax = 1 if (Cw + PASS_COLS - 1) // PASS_COLS <= 1 else 2
    assert (emax == 1) == (We <= E1_WE_MAX)
    DPT = dpt or (1 if max_drops <= NT else 2 if max_drops <= 2 * NT else 4 if max_drops <= 4 * NT else 8)
    rpb = ((He + COL_PARTS - 1) // COL_PARTS + 3) & ~3
    nchunk = (max_drops + NT * DPT - 1) // (NT * DPT)
    nch = 6 if He <= SPANS_H[0] else 8 if He <= SPANS_H[1] else 16
    on_dda = route == 'f32' and dda
    out.update(Cw=Cw, emax=emax, DPT=DPT, rpb=rpb, nchunk=nchunk, per=[-(-n // nchunk) for n in ns],
               empty_bands=[b for b in range(COL_PARTS) if b * rpb >= He], idle_waves=[w for w in range(NT // 64) if w * Cw >= We],
               Hp=(He + 3) & ~3, spans='k_fov_spans<%d, %s>' % (nch, 'true' if on_dda else 'false'))
    out['instances'] = {out['spans'], 'k_fov_sums32<%d, %d, %s>' % (DPT, emax, 'true' if env32 else 'false') if route == 'f32'
                        else 'k_fov_sums<%d, %d>' % (DPT, emax)}
    return out


# ---------------------------------------------------------------------------
# maps
# ---------------------------------------------------------------------------
class Map:
    """An environment map of the catalogue, its float64 prefix table and the bound on the float prefix entries."""
    _cache = {}

    @classmethod
    def get(cls, He, We, env32):
        key = (He, We, bool(env32))
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, He, We, env32):
        self.He, self.We, self.env32 = He, We, env32
        rng = np.random.RandomState(7000 + 31 * He + We)
        env = np.empty((He, We, 3))
        env[..., 0] = rng.uniform(0.2, 0.45, (He, We))
        env[..., 1] = rng.uniform(0.2, 0.45, (He, We))
        env[..., 2] = 10.0 ** rng.uniform(-2.0, 0.0, (He, We))
        env[:, We // 2:, 2] *= 10.0
        omega = h.solid_angle.get_solid_angles(np.zeros((He, We)))
        if env32:                                              # what the library is given, and the same values widened
            self.env_in, self.omega_in = np.ascontiguousarray(env, np.float32), np.ascontiguousarray(omega, np.float32)
        else:
            self.env_in, self.omega_in = np.ascontiguousarray(env), np.ascontiguousarray(omega)
        self.env, self.omega = self.env_in.astype(np.float64), self.omega_in.astype(np.float64)
        self.P = self.prefix(self.env, self.omega)
        self.sumW, self.sumY = float(self.P[:, We, 3].sum()), float(self.P[:, We, 2].sum())
        self._B = {}

    @staticmethod
    def prefix(env, omega):
        He, We = omega.shape
        v = np.concatenate([env * omega[..., None], omega[..., None]], axis=2)       # x w, y w, Y w, w
        P = np.zeros((He, We + 1, 4))
        np.cumsum(v, axis=1, out=P[:, 1:])
        return P

    def entry_bound(self):
        """B[y, j, k]: what entry j (the sum of columns < j) of k_fov_sums32's row y may be off by -- the module's docstring."""
        if 'B' not in self._B:
            emax = 1 if self.We <= E1_WE_MAX else 2
            k = (1 if self.env32 else 3) + 1 + 6 + emax + 4 + 1
            g = k * U / (1 - k * U)
            B = g * self.P
            first = np.arange(1, self.We, 2)                   # through a pair's first column (an even one) with a second behind it
            B[:, first] = g * self.P[:, first + 1] + U * self.P[:, first]
            B[:, 0] = 0.0
            self._B['B'] = B
        return self._B['B']

    def rpb(self):
        return ((self.He + COL_PARTS - 1) // COL_PARTS + 3) & ~3


def span_sums(P, xl, xr):
    """S[n, 4] = sum over the rows of P[y, xr + 1] - P[y, xl]; an empty row (xl > xr) reads (0, 0) like the kernels."""
    He = P.shape[0]
    hi, lo = np.where(xl <= xr, xr + 1, 0), np.where(xl <= xr, xl, 0)
    rows = np.arange(He)[None, :]
    return (P[rows, hi] - P[rows, lo]).sum(axis=1)


def span_bound(mp, xl, xr, S):
    B = mp.entry_bound()
    hi, lo = np.where(xl <= xr, xr + 1, 0), np.where(xl <= xr, xl, 0)
    rows = np.arange(mp.He)[None, :]
    eb = (B[rows, hi] + B[rows, lo]).sum(axis=1)
    r = mp.rpb()
    g = r * U / (1 - r * U)
    return (1 + g) * (1 + U) * eb + (U + g) * S


def xyY_of_sums(S, sumW, sumY):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([S[:, 0] / S[:, 3], S[:, 1] / S[:, 3], GRAY_Y * (0.94 * (S[:, 2] / sumW) + 0.06 * (sumY / sumW))], axis=1)


def xyY_bound(mp, S, dS):
    """Bound on (x, y, Yg) of a drop whose sums are off by at most dS, the whole-map sums by the row totals' bound."""
    B = mp.entry_bound()
    dW, dY = float(B[:, mp.We, 3].sum()), float(B[:, mp.We, 2].sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        r3 = dS[:, 3] / S[:, 3]
        bx = S[:, 0] / S[:, 3] * (dS[:, 0] / S[:, 0] + r3) / (1 - r3)
        by = S[:, 1] / S[:, 3] * (dS[:, 1] / S[:, 1] + r3) / (1 - r3)
    rW = dW / mp.sumW
    bY = GRAY_Y * (0.94 * (dS[:, 2] + S[:, 2] * rW) + 0.06 * (dY + mp.sumY * rW)) / mp.sumW / (1 - rW)
    out = np.stack([bx, by, bY], axis=1)
    return out + 1e-12 * np.abs(xyY_of_sums(S, mp.sumW, mp.sumY))


def reference_sums(case, rule=1):
    """(S[n, 4] float64 per drop, (sum w, sum Y w) of the whole map)."""
    return case.reference_sums(rule)


def rounding_bound(case, rule=1):
    """[n, 3]: what k_fov_sums32's rounding may move (x, y, Yg) of a drop by -- the module's docstring."""
    return case.rounding_bound(rule)


def reference_K(S, sumW, sumY):
    """bad_weather.py:397-412 on a gray value of 1: BGR colour constants [n, 3] of the sums S[n, 4]."""
    xyY = xyY_of_sums(S, sumW, sumY)
    return orc.convert_xyY_to_rgb(xyY)[..., ::-1]


def _xyz_matrix():
    # convert_xyY_to_rgb is XYZ @ M: three points with known XYZ give M
    pts = np.array([[1 / 3, 1 / 3, 1.0], [0.5, 0.25, 1.0], [0.25, 0.5, 1.0]])
    xyz = np.stack([pts[:, 2] * pts[:, 0] / pts[:, 1], pts[:, 2], pts[:, 2] * (1 - pts[:, 0] - pts[:, 1]) / pts[:, 1]], axis=1)
    return np.linalg.solve(xyz, orc.convert_xyY_to_rgb(pts))


_MINV = np.linalg.inv(_xyz_matrix())


def unmix(K):
    """(x, y, Yg)[n, 3] of BGR constants K[n, 3]: XYZ = RGB @ inv(M), x = X / (X + Y + Z), y = Y / (X + Y + Z), Yg = Y."""
    xyz = np.asarray(K, np.float64)[..., ::-1] @ _MINV
    s = xyz.sum(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([xyz[..., 0] / s, xyz[..., 1] / s, xyz[..., 1]], axis=-1)


# ---------------------------------------------------------------------------
# drops
# ---------------------------------------------------------------------------
class Base:
    """What every case shares: the 64 x 128 scene (textures, image), the template records, a camera per cone."""

    def __init__(self, tmp_of):
        import compositor_cases as cc
        self.tpl = cc.Templates(tmp_of('col_tpl'))
        self.scene = h.Scene(tmp_of('col_scene'), IMG_H, IMG_W, 0,
                             frames=[dict(id=0, t=2000, d=0, drops=[h.streak(0, 60, 30, 60, 34, 2.5, 2.5, 6.0, IMG_H, IMG_W)])])
        self.bg, _env = self.scene.frame_inputs(0)
        cs = self.scene.cam_settings
        self.cams = {fov: h.hb.make_camera(cs['focal_mm'] / 1000., cs['f_number'], cs['exposure_ms'], fov=fov) for fov in CONES}
        self.texdb = h.hb.pack_streak_db(self.scene.db.streaks_light)
        self._cases = {}

    TEMPLATE_CYCLE = ('v8', 'v12', 'o9', 'big', 'v3', 'blur', 'v6', 'big2')

    def records(self, n):
        """n records at image positions inside the frame (every footprint non-empty), templates and positions cycling."""
        rows = []
        for i in range(n):
            name = self.TEMPLATE_CYCLE[i % len(self.TEMPLATE_CYCLE)]
            rec, _box = self.tpl.place(name, 8 + (i * 7) % (IMG_W - 32), 6 + (i * 5) % (IMG_H - 34))
            rows.append(rec)
        return np.array(rows, h.hb.DROP_DTYPE)


def aim(drops, az, el, rho):
    """Move the records' world positions: mid-point of wps / wpe at azimuth az (0 ahead, positive to the right), elevation el,
    rho metres from the camera; wps keeps |z| (the plan's depth), wpe takes what the mid-point needs."""
    m = np.stack([rho * np.cos(el) * np.sin(az), rho * np.sin(el), -rho * np.cos(el) * np.cos(az)], axis=1)
    zt = np.abs(drops['wps'][:, 2])
    wps = m + np.array([0.0005, 0.005, 0.0])
    wps[:, 2] = np.where(m[:, 2] <= 0, -zt, zt)
    drops['wps'] = wps
    drops['wpe'] = 2 * m - wps
    return drops


class Case:
    """One frame: map, cone, drop table; ref() is the float64 reference under a fill rule."""

    def __init__(self, base, name, He, We, n, cone=165, env32=True, aims=(), seed=0, lifted=0.15, ties=(), el_max=None):
        self.base, self.name, self.He, self.We, self.n, self.cone, self.env32 = base, name, He, We, n, cone, env32
        self.aims = set(aims)
        self.map = Map.get(He, We, env32)
        self.cam = base.cams[cone]
        rng = np.random.RandomState(9000 + seed)
        drops = base.records(n)
        az = rng.uniform(-np.pi, np.pi, n)
        # the cone's polygon wraps (contains a pole) from an elevation of about 90 - cone / 2 + the parallax of the drop's distance
        calm = np.deg2rad({165: 4.0, 60: 50.0, 12: 80.0}[cone] if el_max is None else el_max)
        el = rng.uniform(-calm, calm, n)
        lift = rng.uniform(0, 1, n) < lifted
        if n:
            lift[0] = lifted > 0                                # (a frame's first drop: the lonely drop of a one-drop frame wraps)
        el = np.where(lift, np.deg2rad(rng.uniform(min(88.0 - cone / 2 + 15.0, 86.0), 89.0, n)) * rng.choice([-1, 1], n), el)
        rho = rng.uniform(1.5, 6.0, n)
        if n and lifted > 0:
            el[0], rho[0] = np.deg2rad(88.0), 2.0
        self.drops = aim(drops, az, el, rho)
        for run in ties:                                       # (first, count): identical records
            self.drops[run[0]:run[0] + run[1]] = self.drops[run[0]]
        self._ref = {}

    # -- what the library is given --
    def frame(self, n=None, bg=None):
        bg = self.base.bg if bg is None else bg
        return dict(bg=bg, rainy_bg=bg, env_xyY=self.map.env_in, omega=self.map.omega_in, drops=self.drops if n is None else self.drops[:n])

    def view(self):
        """The scene as the host build's helpers want it."""
        sc = self.base.scene
        v = type('View', (), {})()
        v.H, v.W, v.He, v.We, v.cam, v.db, v.omega = IMG_H, IMG_W, self.He, self.We, self.cam, sc.db, self.map.omega
        return v

    # -- the reference --
    def polygons(self):
        if 'poly' not in self._ref:
            emu = h.hostemu()
            n = self.n
            texels, hs, ws, offs = self.base.texdb
            plans = np.zeros(max(n, 1), h.PLAN_DTYPE)
            poly, npts, sizes = np.zeros(max(n, 1) * 72, np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64)
            d = np.ascontiguousarray(self.drops)
            emu.emu_plan(h._p(d), n, ctypes.byref(self.cam), IMG_H, IMG_W, self.He, self.We, h._p(hs), h._p(ws), ctypes.c_double(1.0),
                         h._p(plans), h._p(poly), h._p(npts), h._p(sizes))
            self._ref['poly'] = (poly.reshape(-1, 2, 36)[:n], npts[:n], plans[:n], sizes[:n])
        return self._ref['poly']

    def spans_of(self, px, py, rule):
        emu = h.hostemu()
        px, py = np.ascontiguousarray(px, np.int32), np.ascontiguousarray(py, np.int32)
        xl, xr = np.zeros(self.He, np.int32), np.zeros(self.He, np.int32)
        emu.emu_rowspans(h._p(px), h._p(py), len(px), int(self.cam.n_fov), self.He, self.We, int(rule), h._p(xl), h._p(xr))
        return xl, xr

    def spans(self, rule=1):
        """(xl, xr)[n, He] of every drop's polygon (xl > xr: empty; a drop without a polygon: all empty)."""
        key = ('spans', rule)
        if key not in self._ref:
            poly, npts, _plans, _sizes = self.polygons()
            xl, xr = np.ones((self.n, self.He), np.int64), np.zeros((self.n, self.He), np.int64)
            for i in range(self.n):
                if npts[i] > 0:
                    xl[i], xr[i] = self.spans_of(poly[i, 0, :npts[i]], poly[i, 1, :npts[i]], rule)
            self._ref[key] = (xl, xr)
        return self._ref[key]

    def ref(self, rule=1):
        """dict(S[n, 4], K[n, 3], xyY[n, 3], bound[n, 3] (float route), status[n], composited[n] bool)."""
        key = ('ref', rule)
        if key not in self._ref:
            mp = self.map
            xl, xr = self.spans(rule)
            S = span_sums(mp.P, xl, xr)
            poly, npts, plans, sizes = self.polygons()
            status = plans['status'].copy()
            status[(status == 0) & (npts == 0)] = orc.ST_FOV_FAIL
            status[(status == 0) & (npts > 0) & ~(xl <= xr).any(axis=1)] = orc.ST_EMPTY_FOV
            comp = (status == 0) & (sizes > 0)
            K = np.where(comp[:, None], reference_K(S, mp.sumW, mp.sumY), 0.0)
            dS = span_bound(mp, xl, xr, S)
            self._ref[key] = dict(S=S, K=K, xyY=xyY_of_sums(S, mp.sumW, mp.sumY), bound=xyY_bound(mp, S, dS), status=status, composited=comp)
        return self._ref[key]

    def reference_sums(self, rule=1):
        return self.ref(rule)['S'], (self.map.sumW, self.map.sumY)

    def rounding_bound(self, rule=1):
        return self.ref(rule)['bound']

    def features(self, rule=1):
        """Per drop what the catalogue's names promise (bool arrays)."""
        xl, xr = self.spans(rule)
        _poly, npts, _plans, _sizes = self.polygons()
        has = xl <= xr
        r = self.map.rpb()
        top = np.where(has.any(1), has.argmax(1), -1)
        bot = np.where(has.any(1), self.He - 1 - has[:, ::-1].argmax(1), -1)
        f = dict(any=has.any(1), col0=(has & (xl == 0)).any(1), col_last=(has & (xr + 1 == self.We)).any(1), row0=has[:, 0], row_last=has[:, -1],
                 wrap=npts == self.cam.n_fov + 4, one_band=has.any(1) & (top // r == bot // r), narrow=(has & (xr - xl < 8)).any(1),
                 far_right=(has & (xl >= self.We - self.We // 16)).any(1),
                 seam=(has & (10 * (xr - xl + 1) >= 9 * self.We)).any(1) & ~(npts == self.cam.n_fov + 4))       # no pole inside, yet a row nearly the map's width
        for b in range(1, COL_PARTS):
            if b * r < self.He:
                f['straddle_%d' % b] = has[:, b * r - 1] & has[:, b * r]
        return f

    def explain(self, i, got_xyY, rule=1):
        """An exception drop: is the device's (x, y, Yg) within the bound of the reference on a polygon that differs from the float64
        one by one vertex moved one texel in x or y?  Returns the (vertex, dx, dy) that explains it, or None."""
        poly, npts, _plans, _sizes = self.polygons()
        n = int(npts[i])
        mp = self.map
        for k in range(n):
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                px, py = poly[i, 0, :n].copy(), poly[i, 1, :n].copy()
                px[k] += dx
                py[k] += dy
                xl, xr = self.spans_of(px, py, rule)
                xl, xr = xl[None].astype(np.int64), xr[None].astype(np.int64)
                S = span_sums(mp.P, xl, xr)
                if not (xl <= xr).any():
                    continue
                b = xyY_bound(mp, S, span_bound(mp, xl, xr, S))
                if (np.abs(xyY_of_sums(S, mp.sumW, mp.sumY) - got_xyY) <= b).all():
                    return k, dx, dy
        return None

    def emu_status(self, rule=1):
        """Statuses and constants of the host build's whole-frame render (float64 map values)."""
        emu = h.hostemu()
        emu.emu_set_fill_rule(rule)
        try:
            out = h.emu_render(self.view(), self.base.bg, self.base.bg, np.ascontiguousarray(self.map.env), self.drops)
        finally:
            emu.emu_set_fill_rule(1)
        return out['status'], out['K'][:self.n]


# ---------------------------------------------------------------------------
# a float32 restatement of the row scan's STRUCTURE (not of its bits: the contract is the bound)
# ---------------------------------------------------------------------------
def _kogge_stone(v, width):
    """Inclusive scan along the last axis in groups of `width` lanes, float32, log2(width) simultaneous steps."""
    lane = np.arange(v.shape[-1]) % width
    s = 1
    while s < width:
        sh = np.zeros_like(v)
        sh[..., s:] = v[..., :-s]
        v = np.where(lane >= s, v + sh, v).astype(np.float32)
        s *= 2
    return v


def float_prefix(mp):
    """P32[He, We + 1, 4]: the prefix rows as a float32 scan of k_fov_sums32's shape makes them -- products in float, pairs, a
    64-lane scan per pass of 128 columns (rows of 16, then the row totals), the carry between passes, 16 wave totals scanned,
    base + prefix, the pair's first entry as the second minus the second texel."""
    if 'P32' in mp._B:
        return mp._B['P32']
    He, We = mp.He, mp.We
    nw = NT // 64
    Cw = ((We + nw - 1) // nw + 1) & ~1
    emax = (Cw + PASS_COLS - 1) // PASS_COLS
    e32, w32 = mp.env_in.astype(np.float32), mp.omega_in.astype(np.float32)
    v = np.concatenate([e32 * w32[..., None], w32[..., None]], axis=2).astype(np.float32)      # [He, We, 4]
    A = np.zeros((He, 4, nw, emax, 64, 2), np.float32)
    col = np.full((nw, emax, 64, 2), -1)
    for w in range(nw):
        for e in range(emax):
            for s in range(2):
                cl = e * PASS_COLS + 2 * np.arange(64) + s
                c = w * Cw + cl
                ok = (cl < Cw) & (c < We)
                col[w, e, ok, s] = c[ok]
                A[:, :, w, e, ok, s] = v[:, c[ok], :].transpose(0, 2, 1)
    pair = (A[..., 0] + A[..., 1]).astype(np.float32)                                      # [He, 4, nw, emax, 64]
    ps = np.zeros_like(pair)
    carry = np.zeros(pair.shape[:3], np.float32)
    for e in range(emax):
        s = _kogge_stone(pair[:, :, :, e], 16)
        s[..., 16:32] += s[..., 15:16]
        s[..., 48:64] += s[..., 47:48]
        s[..., 32:64] += s[..., 31:32]
        s = (s + carry[..., None]).astype(np.float32)
        ps[:, :, :, e] = s
        carry = s[..., 63]
    wt = _kogge_stone(carry, 16)                                                           # inclusive over the 16 waves
    base = np.zeros_like(wt)
    base[..., 1:] = wt[..., :-1]
    o = (base[..., None, None] + ps).astype(np.float32)
    first = (o - A[..., 1]).astype(np.float32)
    P32 = np.zeros((He, We + 1, 4), np.float32)
    for w in range(nw):
        for e in range(emax):
            ok0, ok1 = col[w, e, :, 0] >= 0, col[w, e, :, 1] >= 0
            P32[:, col[w, e, ok0, 0] + 1, :] = first[:, :, w, e, ok0].transpose(0, 2, 1)
            P32[:, col[w, e, ok1, 1] + 1, :] = o[:, :, w, e, ok1].transpose(0, 2, 1)
    mp._B['P32'] = P32
    return P32


def float_sums(mp, xl, xr):
    """(S[n, 4] float64, sumW, sumY): differences of float_prefix accumulated per band in float32, the bands in float64."""
    P32 = float_prefix(mp)
    hi, lo = np.where(xl <= xr, xr + 1, 0), np.where(xl <= xr, xl, 0)
    r = mp.rpb()
    S = np.zeros((len(xl), 4))
    for b in range(COL_PARTS):
        acc = np.zeros((len(xl), 4), np.float32)
        for y in range(b * r, min(mp.He, (b + 1) * r)):
            acc = (acc + (P32[y, hi[:, y]] - P32[y, lo[:, y]]).astype(np.float32)).astype(np.float32)
        S += acc.astype(np.float64)
    return S, float(P32[:, mp.We, 3].astype(np.float64).sum()), float(P32[:, mp.We, 2].astype(np.float64).sum())


# ---------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------
WIDTHS = ((64, 20), (64, 21), (64, 254), (64, 255), (64, 256), (64, 2047), (64, 2048), (64, 2049), (16, 4095), (16, 4096))
HEIGHTS = (20, 63, 64, 384, 385, 512, 513, 1024, 1025)
HEIGHTS_WE = 96
N_SMALL = 256
BIG_N = 8193
# the big table's runs of identical records (ties): around the chunk boundaries of 2500 drops in three chunks (834, 1668) and
# of 8193 in two (4097) in table order, next to each other and far apart
BIG_TIES = ((830, 8), (1664, 8), (4092, 10), (100, 3))
DPT_CASES = tuple((d, 1024 * d + k) for d in (1, 2) for k in (-1, 0, 1)) + ((4, 4096), (8, 8192), (1, 2500))
BATCH_NS = (0, 1, 1025, 2500)
PLACEMENT_MAPS = ((64, 255), (16, 4096))


def width_name(He, We, cone, env32):
    return 'w%dx%d_c%d_%s' % (He, We, cone, 'f32' if env32 else 'f64')


def build(base):
    """name -> Case.  Built once per process (Base caches it)."""
    if base._cases:
        return base._cases
    c = {}
    for k, (He, We) in enumerate(WIDTHS):
        for cone in (165, 60):
            for env32 in (True, False):
                aims = {'width'} | ({'odd_width'} if We % 2 else set()) | ({'idle_waves'} if We == 20 else set())
                c[width_name(He, We, cone, env32)] = Case(base, width_name(He, We, cone, env32), He, We, N_SMALL, cone, env32, aims, seed=k)
    for k, He in enumerate(HEIGHTS):
        c['h%d' % He] = Case(base, 'h%d' % He, He, HEIGHTS_WE, N_SMALL, 165, True, {'height'}, seed=100 + k)
    c['h1025_f64'] = Case(base, 'h1025_f64', 1025, HEIGHTS_WE, N_SMALL, 165, False, {'height'}, seed=120)
    c['big'] = Case(base, 'big', 64, 255, BIG_N, 165, True, {'chunks', 'order', 'odd_width'}, seed=200, ties=BIG_TIES)
    for He, We in PLACEMENT_MAPS:
        for cone in CONES:
            name = 'place%dx%d_c%d' % (He, We, cone)
            c[name] = Case(base, name, He, We, 320, cone, True, {'placement'} | ({'odd_width'} if We % 2 else set()), seed=300 + cone + We,
                           lifted=0.1, el_max={165: 12.0, 60: 58.0, 12: 83.0}[cone])
    base._cases = c
    return c


def width_cases():
    return [width_name(He, We, cone, env32) for He, We in WIDTHS for cone in (165, 60) for env32 in (True, False)]


def runs():
    """Every call the GPU tier makes, as predict() sees it: (case name, drop counts, dict(route, dpt, dda, env32))."""
    out = []
    for He, We in WIDTHS:
        for cone in (165, 60):
            for env32 in (True, False):
                for route in ('f32', 'f64'):
                    out.append((width_name(He, We, cone, env32), (N_SMALL,), dict(route=route, env32=env32)))
    for env32 in (True, False):                                   # every drops-per-thread instance on both widths' classes
        for We in (255, 2049):
            for dpt in (1, 2, 4, 8):
                for route in ('f32', 'f64'):
                    out.append((width_name(64, We, 165, env32), (N_SMALL,), dict(route=route, env32=env32, dpt=dpt)))
    for He in HEIGHTS:
        for route, dda in (('f32', 1), ('f32', 0), ('f64', 1)):
            out.append(('h%d' % He, (N_SMALL,), dict(route=route, dda=dda)))
    out.append(('h1025_f64', (N_SMALL,), dict(route='f32', env32=False)))
    for dpt, n in DPT_CASES:
        for route in ('f32', 'f64'):
            out.append(('big', (n,), dict(route=route, dpt=dpt)))
    out.append(('big', (BIG_N,), dict(route='f32')))
    out.append(('big', (BIG_N,), dict(route='f64')))
    out.append(('big', BATCH_NS, dict(route='f32', dpt=1)))
    out.append(('big', BATCH_NS, dict(route='f32')))
    for He, We in PLACEMENT_MAPS:
        for cone in CONES:
            out.append(('place%dx%d_c%d' % (He, We, cone), (320,), dict(route='f32')))
    return out


def surrogate_order(case, n, rule=1):
    """A stand-in for k_fov_sort's order (its key is k_fov_vertices' own): the drops of table[:n] by the top row of their spans,
    ties in table order.  Only used to model a list drop written at its index instead of its slot."""
    xl, xr = case.spans(rule)
    has = (xl <= xr)[:n]
    top = np.where(has.any(1), has.argmax(1), case.He)
    return np.argsort(top, kind='stable')
