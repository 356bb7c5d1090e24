"""The fog and environment-map pre-pass (csrc/rr_prepass.h, enqueue_prepass in rainhip.hip) against a float64 reference: a
catalogue of frame sizes, inputs, element types and tap counts aimed at the places where k_fog_sum / k_fog_mean /
k_fog_tile<12> (or k_fog_ext / k_fog_h / k_fog_v) and k_env_build / k_env_h / k_env_v branch, the reference, and bounds on what
the kernels may differ by, counted from the code.  tests/test_prepass_cases_host.py runs the catalogue through the host build of
the same functions (tests/hostemu), tests/test_gpu_prepass_cases.py through RainHip.prepass_frames.

The reference (ref_fog, ref_env_map) is oracle.prepass.fog_rain_layer / generate_env_map with the two tap vectors as parameters
(scipy.ndimage.correlate1d, mode='mirror'); for 25 and 15 taps it is the oracle, bit for bit (asserted on the host tier).  The
float32-depth path keeps numpy's float32 semantics (depth / 1000, weak scalar times float32) as the oracle has them.  A float32
image is taken at its own values widened, a uint8 image as bytes / 255.0 (rr_prepass.h load_unit; generator.py:352); uint16 depth
samples are float32 metres = sample / 256 (generator.py:366).

Inputs.  helpers.prepass_scene (depths of 2 to 83 m: no clamp acts) and a saturating scene made from it (saturating()): rain
intensity 200, image rows [:H//2] = 1.0, the left half of the other rows 0.0, depth 0 m in the left quarter of the columns and
1e6 m in the right quarter.  A fog value is exactly 0 only where the image is 0 and the blurred l_in is 0, that is where the whole
blur window has 1 - f_ext <= 0: the left quarter must be wider than half a window (HALF columns, 16 for 33 taps).  Narrower
frames (every catalogue size but 72 x 257) get a hand-written depth instead: -50 m (an invalid-sample marker: f_ext = e^0.54 > 1, so 1 - f_ext < 0 and clip01 cuts
l_in at 0 -- the branch no non-negative depth ever takes -- and image * f_ext > 1 is cut at 1) in the left half of the columns,
or in all of them where the frame is narrower than two windows; the 1e6 m quarter stays where it does not overlap.  The fog-only
sizes (one row or one column) take -50 m everywhere and an image of channels (1, 0, scene).  What a saturating, white or black
input must reach is asserted from the reference alone (Case.assert_reaches_clamps) before any kernel output is looked at.

Bounds -- every rounding is charged eps = 2^-53 times the largest magnitude S the case's planes reach (1 for inputs in [0, 1] and
k3 <= 1); a rounding to nearest of a value below S moves it by at most S eps / 2, so a count of the kernel's operations at eps
each also pays for the reference's chain of the same length.

bound_f64 (float64 depth; image * f_ext + l_in, both blurred twice):
    exp                                   2   one ulp for each libm (the argument is formed by the same operations)
    1 - f_ext                             1
    the channel mean                      A + 1 + e_ref + 2
        A = ceil(px / 16384) + 8 + 64: the additions a term of k_fog_sum / k_fog_mean passes through (a thread's strided terms,
        the tree of 256, the 64 blocks; tests/hostemu sums in the same order); 1 the division; e_ref the relative error of the
        reference's own np.mean -- numpy adds the rows one after the other here, so it is MEASURED per case against math.fsum
        (correctly rounded; + 2 for fsum's own rounding and its division)
    k3 = beta_hg * mean, k3 * (1 - f_ext) 2
    a blur pass                           P = (half + 1) + 2 half + 1: the products, the additions, and the weights' sum != 1
    four passes                           4 P  (two for f_ext, two for l_in; a convex blur does not amplify what it is given)
    image * f_ext + l_in                  2
  k = 10 + A + e_ref + 4 P: 10 + 74 + e_ref + 152 for 25 taps at 72 x 257, about 3e-14 with e_ref of a few tens.  No case may pass
  1e-12 (asserted): above it a float32 rounding slipped into this path -- at least 6e-8 times the image value -- would stop
  being a certain failure.  The largest in the catalogue is 2.4e-13, the saturating scene at 72 x 257: its e_ref is 1516 (half
  the terms are the same 1145.9..., and numpy's row-by-row sum drifts one way), and the difference seen there, 7.6e-14, is the
  reference's own.  (Seen on the host build and on the device for the suite's scene: 2.7e-15 at most.  Notes, not the source
  of the bound.)

bound_f32 (float32 or uint16 depth), u = 2^-24, the float32 ulp below 1 (the next binade's where f_ext > 1):
  Assumption about the libms: ocml's expf (and glibc's, on the host tier) returns one of the two float32 neighbours of the
  true value (an error below 1 ulp: faithful).  numpy's expf is not taken on trust (its SIMD loops are documented to a few ulp;
  1.4 ulp was seen here): it is MEASURED per pixel against float64 exp of the same float32 argument, e_s ulp.  The two results
  are floats, so they differ by a whole number of ulps below 1 + e_s: d_s = floor(1 + e_s), which is 1 wherever numpy is
  faithful too and never more than the 2 ulp that two 1-ulp error bars add up to unless numpy itself is worse than that.  The
  blurs are convex, so what reaches an output pixel is at most d = max over the pixels of blur(d_s), with the case's own taps.
    f_ext differs by delta, |delta| <= d_s u.  1 - f_ext differs by -delta + rho; rho = 0 where 0.5 <= f_ext <= 2 for the whole
    case (the subtraction is exact), else |rho| <= u (half an ulp per side).  l_in = clip(k3 (1 - f_ext)) moves by
    theta k3 (-delta + rho) with 0 <= theta <= 1 (the clip is monotone and 1-Lipschitz), and both blurs are convex, so in
    image * f_ext + l_in a source pixel's delta is weighted by (image - theta k3), between -k3 and image:
        d u max(image_max, k3) + r_om u k3
    the (double)(float) of plane 0 after each of its two passes: half an ulp per side and pass
        2 u image_max
    and everything the float64 chain adds: bound_f64.
  For helpers.prepass_scene (image_max 0.8, k3 0.85 .. 1.1) this is 1.5e-7 to 1.7e-7, below the suite's 2e-7 (asserted).

The map.  The uint8 map must equal ref_env_map of the kernel's OWN fog output bit for bit (so that only map logic is compared),
and xyY must be within 1e-12 of oracle.prepass.env_to_xyY of it.  For float64 depth the map made from the REFERENCE's fog layer
is compared too: a byte (rainy * 255).astype(uint8) can differ only where the reference's rainy * 255 lies within 255 bound_f64
of an integer (risky_pixels), and a map cell only where such a pixel is gathered, filled in or blurred into it (cells_of)."""
import functools
import importlib
import math

import numpy as np
from scipy.ndimage import correlate1d, maximum_filter1d

import helpers as h
from oracle import prepass as op

fogmod = importlib.import_module('rain-rendering_amd.common.add_attenuation')
envmod = importlib.import_module('rain-rendering_amd.common.envmap')

FOCAL, FNUM, EXPO, GAIN = 0.006, 6.0, 2, 20
EPS = 2.0 ** -53
U32 = 2.0 ** -24
F64_LIMIT = 1e-12                      # no float64 bound may pass this
SUITE_F32 = 2e-7                       # the suite's float32 allowance (tests/test_gpu_prepass.py)
XYY_TOL = 1e-12

# rr_prepass.h: FogTile<12> and the launches of enqueue_prepass
TC, RB, VR, HALF, FOG_SEG = 32, 8, 4, 12, 256
FOG_BLOCKS, FOG_THREADS = 64, 256
TILE_TAPS = 25                         # `const bool tiled = ctx->pk.fog_k == 25;`


def tile_seg_rows(H, W, n=1):
    """enqueue_prepass: the rows of a k_fog_tile segment for a batch of n frames (segments are cut while each keeps 64 rows)."""
    strips = (W + TC - 1) // TC
    segs = 1
    while strips * n * segs < 3072 and H // (segs + 1) >= 64:
        segs += 1
    return ((H + segs - 1) // segs + RB - 1) // RB * RB


# (H, W): what the size hits
FOG_ONLY_SIZES = [
    (1, 1),      # a single pixel: every reflection returns 0, one thread of one block has a term of the mean
    (1, 40),     # one row: the vertical window is that row 25 times; a second strip of 8 columns
    (40, 1),     # one column: the horizontal window is that column; strips one column wide
]
MAP_SIZES = [
    (2, 3),      # the smallest size the map geometry accepts (focal length 1); We = 5
    (9, 5),      # smaller than the 12-pixel border both ways: reflect101 bounces
    (13, 33),    # one past HALF; the second strip is one column wide
    (25, 31),    # one window high, a strip one column short
    (65, 33),    # the last block of 8 rows holds one row
    (128, 32),   # two segments of exactly 64 rows
    (129, 33),   # two segments; the second is 57 rows: 1 mod 8 and 1 mod 4
    (192, 32),   # three segments; the middle one has both neighbours
    (72, 257),   # We = 393: a partial second 256-cell block in the three map kernels; k_fog_h has a second segment of one column
]
TAP_COUNTS = [(25, 15), (1, 1), (3, 3), (9, 33), (33, 9), (25, 33), (25, 1)]          # (fog, map); 25 fog taps: k_fog_tile
TAP_SIZES = [(25, 31), (72, 257)]
TYPE_SIZE = (65, 33)                   # every image type with every depth type
FLAT_SIZE = (25, 31)                   # the all-white and the all-black image
IMG_TYPES = (np.float64, np.float32, np.uint8)
DEPTH_TYPES = (np.float64, np.float32, np.uint16)


def fog_taps(n):
    return np.array([1.0]) if n == 1 else op.gaussian_kernel(n, n)          # (25, 25) for the reference's own count


def env_taps(n):
    return np.array([1.0]) if n == 1 else op.gaussian_kernel(n, 0)          # (15, 0)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def _blur(img, w):
    out = correlate1d(img, w, axis=1, mode='mirror')
    return correlate1d(out, w, axis=0, mode='mirror')


def widen(image):
    """The float64 image the kernels compute with (load_unit)."""
    image = np.asarray(image)
    return image / 255.0 if image.dtype == np.uint8 else image.astype(np.float64)


def metres(depth):
    """uint16 samples -> float32 metres (depth_f32_at); float maps as they are."""
    depth = np.asarray(depth)
    return depth.astype(np.float32) / np.float32(256.) if depth.dtype == np.uint16 else depth


def fog_parts(image, depth, rain, fog_w):
    """oracle.prepass.fog_rain_layer with the taps as a parameter; returns the layer and the quantities the bounds are made of."""
    image, depth = widen(image), metres(depth)
    beta_ext, beta_hg, _ = op.fog_constants(rain, FNUM, EXPO, GAIN)
    fe = np.exp((-beta_ext) * (depth / 1000))
    f_ext = np.tile(np.expand_dims(fe, axis=-1), (1, 1, 3))
    irradiance = (4 * (FNUM ** 2) * image) / ((EXPO * 1e-3) * GAIN * np.pi)
    irradiance_mean = np.mean(irradiance.reshape(-1, 3), axis=0)
    om = 1 - f_ext
    l_in = np.clip(beta_hg * irradiance_mean * om, 0, 1)
    f_ext = _blur(f_ext, fog_w)
    l_in = _blur(l_in, fog_w)
    rainy = np.clip(np.clip(image * f_ext + l_in, 0, 1), 0, 1)
    return dict(rainy=rainy, fe=fe, om=om, k3=beta_hg * irradiance_mean, irradiance=irradiance, mean=irradiance_mean,
                image=image, depth=depth, beta_ext=beta_ext)


def ref_fog(image, depth, rain, fog_w):
    return fog_parts(image, depth, rain, fog_w)['rainy']


def _env_assemble(bg8, focal_m):
    """oracle.prepass.generate_env_map up to its blur: the map with its unfilled cells still empty, and the mask of filled cells."""
    H, W = bg8.shape[:2]
    cw, uniq, first = op.env_geometry(focal_m, H, W)
    cyl = np.zeros((H, cw, 3), np.uint8)
    cyl.reshape(-1, 3)[uniq] = bg8.reshape(-1, 3)[first]
    mask = np.zeros((H, cw), np.uint8)
    mask.reshape(-1)[uniq] = 255
    half = H // 2
    fl, mfl = cyl[::-1], mask[::-1]
    tmp = fl[:half].copy()
    r, c = np.nonzero(mfl[:half] == 0)
    src = np.argmax(mask[half:][::-1] > 0, axis=0)
    tmp[r, c] = fl[src[c], c]
    if half:
        cyl[-half:] = tmp[::-1]
    r, c = np.nonzero(mask[:half] == 0)
    src = np.argmax(mask[:half] > 0, axis=0)
    cyl[r, c] = cyl[src[c], c]
    lw = int(cw / 2)
    result = np.zeros((H, cw + 2 * lw, 3), np.uint8)
    result[:, lw:lw + cw] = cyl
    mres = np.zeros((H, cw + 2 * lw), np.uint8)
    mres[:, lw:lw + cw] = mask
    side = cyl[:, 0:lw][:, ::-1]
    result[:, 0:side.shape[1]] = side
    mside = mask[:, :cw // 2][:, ::-1]
    mres[:, :mside.shape[1]] = mside
    side = cyl[:, cw // 2:][:, ::-1]
    result[:, result.shape[1] - side.shape[1]:] = side
    mside = mask[:, cw // 2:][:, ::-1]
    mres[:, mres.shape[1] - side.shape[1]:] = mside
    return result, mres


def ref_env_map(background, env_w, focal_m=FOCAL):
    """oracle.prepass.generate_env_map with the taps as a parameter; the BGR float map in [0, 1]."""
    result, mres = _env_assemble((background * 255).astype(np.uint8), focal_m)
    blur = np.clip(np.rint(_blur(result.astype(np.float64), env_w)), 0, 255).astype(np.uint8)
    return np.where(mres[..., None] == 0, blur, result) / 255.0


def map_bytes(env_bgr):
    return np.rint(env_bgr * 255).astype(np.uint8)


def risky_pixels(rainy_ref, bound):
    """Pixels with a channel whose rainy * 255 lies within 255 * bound of an integer: a fog layer within `bound` of the
    reference's may give another byte there, and nowhere else."""
    v = rainy_ref * 255
    return (np.abs(v - np.rint(v)) <= 255 * bound).any(axis=-1)


def cells_of(pixels, n_env_taps, focal_m=FOCAL):
    """The map cells a set of image pixels (bool H x W) can reach: gathered or filled-in copies, and the unfilled cells
    whose blur window holds one."""
    marker = np.repeat(pixels[..., None], 3, axis=-1).astype(np.uint8) * 255
    result, mres = _env_assemble(marker, focal_m)
    hit = result.any(axis=-1).astype(np.uint8)
    spread = maximum_filter1d(maximum_filter1d(hit, n_env_taps, axis=1, mode='mirror'), n_env_taps, axis=0, mode='mirror')
    return np.where(mres == 0, spread, hit) > 0


# ---------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------
def mean_chain(px):
    """The additions a term passes through in k_fog_sum (a thread's strided terms, the tree of 256) and k_fog_mean (64 blocks)."""
    return -(-px // (FOG_BLOCKS * FOG_THREADS)) + 8 + FOG_BLOCKS


def ref_mean_error(parts):
    """The relative error of the reference's own channel means in units of 2^-53, measured against math.fsum."""
    irr = parts['irradiance'].reshape(-1, 3)
    worst = 0.0
    for c in range(3):
        exact = math.fsum(irr[:, c]) / irr.shape[0]
        if exact != 0.0:
            worst = max(worst, abs(parts['mean'][c] - exact) / exact / EPS)
    return math.ceil(worst) + 2


def magnitude(parts):
    """S: the largest magnitude a plane of the case reaches (1 for inputs in [0, 1] with k3 <= 1)."""
    k3 = float(parts['k3'].max())
    return max(1.0, k3, float(parts['fe'].max()), k3 * float(np.abs(parts['om']).max()))


def bound_f64_count(parts, n_fog_taps):
    half = n_fog_taps // 2
    P = (half + 1) + 2 * half + 1
    px = parts['fe'].size
    return 2 + 1 + (mean_chain(px) + 1 + ref_mean_error(parts)) + 2 + 4 * P + 2


def bound_f64(parts, n_fog_taps):
    """|kernel - reference| of the fog layer on the float64-depth path (see the module's docstring for the count)."""
    assert parts['image'].min() >= 0.0 and parts['image'].max() <= 1.0
    return bound_f64_count(parts, n_fog_taps) * magnitude(parts) * EPS


def ref_expf_error(parts):
    """numpy's float32 exp on the case's own arguments against float64 exp: per pixel, in float32 ulps of the true value."""
    depth = parts['depth']
    assert depth.dtype == np.float32 and parts['fe'].dtype == np.float32
    arg = (-parts['beta_ext']) * (depth / 1000)
    assert arg.dtype == np.float32
    true = np.exp(arg.astype(np.float64))
    ulp = np.maximum(np.spacing(true.astype(np.float32)).astype(np.float64), 2.0 ** -48)       # (results that underflow: absolute)
    return np.abs(parts['fe'].astype(np.float64) - true) / ulp


def bound_f32(parts, n_fog_taps):
    """|kernel - reference| of the fog layer on the float32-depth path (see the module's docstring)."""
    d = float(_blur(np.floor(1.0 + ref_expf_error(parts)), fog_taps(n_fog_taps)).max())
    fe = parts['fe']
    r_om = 0 if (fe.min() >= 0.5 and fe.max() <= 2.0) else 1
    u = U32 if fe.max() <= 1.0 else float(np.spacing(np.float32(fe.max())))
    k3, img = float(parts['k3'].max()), float(parts['image'].max())
    return u * (d * max(img, k3) + r_om * k3 + 2 * img) + bound_f64(parts, n_fog_taps)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
SEED = 3


def narrow_image(bg, dtype):
    """bg as `dtype`: float32 rounds, uint8 truncates as the frame readers do (1.0 -> 255, 0.0 -> 0)."""
    if dtype == np.uint8:
        return (bg * 255).astype(np.uint8)
    return bg.astype(dtype)


def saturating(H, W, half=HALF):
    """(image, float64 depth, hand) of the saturating scene for a fog blur of 2 half + 1 taps; hand: the depth is the
    hand-written one (module docstring)."""
    bg, depth = h.prepass_scene(H, W, SEED, np.float64)
    bg = bg.copy()
    if H == 1 or W == 1:                          # fog-only sizes: the clamps by channel
        bg[..., 0], bg[..., 1] = 1.0, 0.0
        depth[:] = -50.0
        return bg, depth, True
    bg[:H // 2] = 1.0
    bg[H // 2:, :W // 2] = 0.0
    if W // 4 > half:
        depth[:, :W // 4] = 0.0
        depth[:, W - W // 4:] = 1e6
        return bg, depth, False
    nz = W if W < 2 * (half + 1) else W // 2
    depth[:, :nz] = -50.0
    if nz < W:
        depth[:, W - W // 4:] = 1e6
    return bg, depth, True


def depth_u16(H, W):
    """uint16 depth samples (metres * 256) holding both ends of the type."""
    rng = np.random.RandomState(4)
    d16 = (np.linspace(80, 2, H)[:, None] * np.ones((1, W)) * 256 + rng.uniform(0, 700, (H, W))).astype(np.uint16)
    d16.flat[0], d16.flat[-1] = 0, 65535
    if d16.size > 2:
        d16.flat[d16.size // 2] = 65535
        d16.flat[1] = 0
    return d16


class Case:
    """One frame of the catalogue.  kind: 'scene' | 'sat' | 'white' | 'black'."""

    def __init__(self, H, W, kind, img_t, depth_t, taps=(25, 15), want_env=True):
        self.H, self.W, self.kind, self.img_t, self.depth_t, self.taps, self.want_env = H, W, kind, img_t, depth_t, taps, want_env
        self.rain = 200 if kind in ('sat', 'white', 'black') else 50
        self.name = '%dx%d-%s-%s-%s-%d.%d' % (H, W, kind, np.dtype(img_t).name, np.dtype(depth_t).name, taps[0], taps[1])
        self.f64 = np.dtype(depth_t) == np.float64
        self.tiled = taps[0] == TILE_TAPS

    def __repr__(self):
        return self.name

    @functools.cached_property
    def inputs(self):
        H, W = self.H, self.W
        if self.kind == 'sat':
            bg, depth, _ = saturating(H, W, max(HALF, self.taps[0] // 2))
        else:
            bg, depth = h.prepass_scene(H, W, SEED, np.float64)
            if self.kind == 'white':
                bg = np.ones_like(bg)
            elif self.kind == 'black':
                bg = np.zeros_like(bg)
        depth = depth_u16(H, W) if self.depth_t == np.uint16 else depth.astype(self.depth_t)
        bg = np.ascontiguousarray(narrow_image(bg, self.img_t))
        bg.setflags(write=False)
        depth.setflags(write=False)
        return bg, depth

    @functools.cached_property
    def parts(self):
        p = fog_parts(*self.inputs, self.rain, fog_taps(self.taps[0]))
        for v in p.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return p

    @property
    def rainy(self):
        return self.parts['rainy']

    @functools.cached_property
    def bound(self):
        return bound_f64(self.parts, self.taps[0]) if self.f64 else bound_f32(self.parts, self.taps[0])

    @functools.cached_property
    def ref_map(self):
        """The uint8 map of the reference's own fog layer."""
        m = map_bytes(ref_env_map(self.rainy, env_taps(self.taps[1])))
        m.setflags(write=False)
        return m

    def fog_consts(self):
        return fogmod.FogRain(rain_intensity=self.rain, focal=FOCAL, f_number=FNUM, angle=90, exposure=EXPO, camera_gain=GAIN).constants()

    def frame(self):
        bg, depth = self.inputs
        return dict(bg_u8=bg, depth=depth, fog=self.fog_consts()) if bg.dtype == np.uint8 else dict(bg=bg, depth=depth, fog=self.fog_consts())

    # -- what the input must reach, from the reference alone ----------------
    def assert_reaches_clamps(self):
        """A saturating input has fog values equal to 0, equal to 1, and a map cell of three zero bytes; a black image the
        first and the last, a white one the second.  From the reference alone: a case that does not reach its clamps is a
        failure of the catalogue."""
        if self.kind == 'scene':
            return None
        r = self.rainy
        n0, n1 = int((r == 0.0).sum()), int((r == 1.0).sum())
        nb = int((self.ref_map == 0).all(axis=-1).sum()) if self.want_env else None
        if self.kind in ('sat', 'black'):
            assert n0 > 0, (self.name, 'no fog value equal to 0')
            assert nb is None or nb > 0, (self.name, 'no black map cell')
        if self.kind in ('sat', 'white'):
            assert n1 > 0, (self.name, 'no fog value equal to 1')
        return n0, n1, nb

    # -- the comparisons ------------------------------------------------------
    def check_fog(self, rainy, rainy_f32=None):
        assert rainy.dtype == np.float64 and rainy.shape == self.rainy.shape
        d = float(np.abs(rainy - self.rainy).max())
        assert d <= self.bound, (self.name, 'fog layer', d, self.bound)
        if rainy_f32 is not None:
            assert rainy_f32.dtype == np.float32 and np.array_equal(rainy_f32, rainy.astype(np.float32)), (self.name, 'float32 fog layer')
        return d

    def check_map(self, rainy, env_u8, env_xyY, env_xyY_f32=None, env_u8_f32=None, expect_ref_map=False):
        """env_u8 / env_xyY: the kernels' maps made from their own fog layer `rainy`."""
        ew = env_taps(self.taps[1])
        e_bgr = ref_env_map(rainy, ew)
        want8 = map_bytes(e_bgr)
        assert env_u8.shape == want8.shape, (self.name, env_u8.shape, want8.shape)
        assert np.array_equal(env_u8, want8), (self.name, 'uint8 map', int((env_u8 != want8).any(axis=-1).sum()))
        want_xyY = op.env_to_xyY(e_bgr)
        assert not np.isnan(env_xyY).any(), (self.name, 'nan in xyY')
        dx = float(np.abs(env_xyY - want_xyY).max())
        assert dx < XYY_TOL, (self.name, 'xyY', dx)
        if self.kind in ('sat', 'black'):
            black = (want8 == 0).all(axis=-1)
            assert black.any() and (env_xyY[black] == 0.0).all(), (self.name, 'xyY of a black cell')
        if env_xyY_f32 is not None:
            assert env_xyY_f32.dtype == np.float32 and np.array_equal(env_xyY_f32, env_xyY.astype(np.float32)), (self.name, 'float32 xyY')
        if env_u8_f32 is not None:
            assert np.array_equal(env_u8_f32, env_u8), (self.name, 'uint8 map of the float32 call')
        if self.f64:
            differs = (env_u8 != self.ref_map).any(axis=-1)
            allowed = cells_of(risky_pixels(self.rainy, self.bound), len(ew))
            assert not (differs & ~allowed).any(), (self.name, 'map of the reference fog layer', int((differs & ~allowed).sum()))
            if expect_ref_map:
                assert not differs.any(), (self.name, 'map differs from the reference map', int(differs.sum()))
        return dx


def _rot(seq, i):
    return seq[i % len(seq)]


@functools.lru_cache(maxsize=None)
def catalogue():
    """Every case, in the order of the sizes.  Per map size: the scene on both depth paths, the saturating scene on both, uint16
    depth; the image types rotate over the sizes, and TYPE_SIZE has all nine pairs.  FLAT_SIZE adds the flat images, TAP_SIZES the
    other tap counts, the fog-only sizes run without a map."""
    cases = []
    for H, W in FOG_ONLY_SIZES:
        for kind in ('scene', 'sat'):
            for dt in (np.float64, np.float32):
                cases.append(Case(H, W, kind, np.float64, dt, want_env=False))
        cases.append(Case(H, W, 'scene', np.uint8, np.uint16, want_env=False))
    for i, (H, W) in enumerate(MAP_SIZES):
        cases.append(Case(H, W, 'scene', np.float64, np.float32))
        cases.append(Case(H, W, 'scene', _rot(IMG_TYPES, i), np.float64))
        cases.append(Case(H, W, 'sat', np.float64, np.float64))
        cases.append(Case(H, W, 'sat', _rot(IMG_TYPES, i + 1), np.float32))
        cases.append(Case(H, W, 'scene', _rot(IMG_TYPES, i + 2), np.uint16))
        if (H, W) == TYPE_SIZE:
            cases += [Case(H, W, 'scene', it, dt) for it in IMG_TYPES for dt in DEPTH_TYPES]
        if (H, W) == FLAT_SIZE:
            cases += [Case(H, W, kind, np.float64, dt) for kind in ('white', 'black') for dt in (np.float64, np.float32)]
        if (H, W) in TAP_SIZES:
            for taps in TAP_COUNTS:
                cases.append(Case(H, W, 'scene', np.float64, np.float32, taps))
                cases.append(Case(H, W, 'sat', np.float64, np.float64, taps))
    seen, out = set(), []
    for c in cases:
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return tuple(out)


def sizes():
    return FOG_ONLY_SIZES + MAP_SIZES


def cases_of(H, W):
    return [c for c in catalogue() if (c.H, c.W) == (H, W)]
