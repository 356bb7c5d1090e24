"""Rain on PyTorch image batches that already live on the GPU: the augmentation form of the renderer.

    aug = RainAugment(dataset='kitti', streaks_db='3rdparty/rainstreakdb', sequence='data_object/training')
    rainy, mask = aug(images, depth, intensity=25, frame_index=idx)

`images` is [B, 3, H, W] RGB on the GPU, uint8 (torchvision.io.decode_png) or float32 in [0, 1] (ToTensor); `depth` is
[B, H, W] or [B, 1, H, W] float32 metres.  `rainy` comes back like `images` (same dtype and layout), `mask` as float32
[B, 1, H, W] (rainy_mask).  float16 and bfloat16 batches are taken too: a value enters as the float32 it equals, and `rainy` is the
float32 result rounded once to the batch's dtype.  A channels-last batch (`x.to(memory_format=torch.channels_last)`, or a decoder's
[B, H, W, 3] frames seen as `.permute(0, 3, 1, 2)`) is read where it lies and `rainy` comes back with the same strides, the same values
as the planar call; any other striding is made planar-contiguous first and comes back planar.
Image i is rendered as frame frame_index[i] of a `main.py --device_particles` run on that dataset and sequence at its intensity:
simulated frame f % n_sim, drawn with seed f (generator.py:304-321).  The uint8 result is the RGB of the PNG that run writes; the float32 result is that byte / 255, what ToTensor makes of the file.

`particle_model='field'` (default 'iid') renders the frames of a `main.py --device_particles --particle_model field` run instead:
a persistent particle field (tools/particles.py) in which frame f + 1 shows the drops of frame f a little lower and closer.
`frame_index[i]` is then the TIME index of image i (time f / cam_hz, settings of simulated frame f % n_sim), so a video clip of T
frames is `frame_index = k0 + arange(T)`; a [B, T, 3, H, W] batch is flattened to [B * T, 3, H, W] with one index per frame
(INTEGRATION.md section C).  Frames remain random-access: any index, in any batch, gives the same bits.

`particle_model='rig'` with `rig=Rig...` (rig.py) renders the cameras of a rig looking at ONE such field (stereo, surround): `images`
is [B, V, 3, H, W], `depth` [B, V, H, W] or [B, V, 1, H, W], with one `frame_index` (the instant) and one `intensity` per B; `rainy`
comes back [B, V, 3, H, W], `mask` [B, V, 1, H, W].  View v of instant f is frame f of a `main.py --device_particles
--particle_model rig --rig ... --rig_view v` run.  `views=[...]` restricts the call to a subset of the rig's views (V = len(views),
in that order) with the same bits per view.

`trajectory=Trajectory...` (trajectory.py; needs `particle_model='rig'`, a single camera is `rig=Rig.from_spec('mono')`) moves and
turns the rig through the field: `frame_index[i]` also selects the pose (an index outside the trajectory is a ValueError), the streak
is the drop's path relative to the camera over the exposure, and the frames are those of a `main.py ... --trajectory FILE` run.
`set_trajectory()` swaps the trajectory between batches.

`draws='counter'` (default 'stream') takes every drop's texture pick from the drop's own Philox counter instead of the run's numpy
stream (tools/particles.py, `main.py --particle_draws counter`): under 'field' and 'rig' a drop then keeps its streak pattern in every
frame of its life and in every view, and the device skips its one serial pass (0.15 ms of a KITTI 25 mm/hr call).  The frames are those of
a `--particle_draws counter` run; 'stream' remains the mode that matches a run that writes the reference's files.

`jitter=DEG` (default 0: off) turns every streak by DEG degrees times a standard normal deviate of the drop's own, taken from the
drop's Philox counter (tools/particles.py counter_jitter, `main.py --streak_jitter DEG`): streaks no longer all line up with the
projected fall direction, and under 'field' and 'rig' a drop keeps its tilt in every frame of its life and in every view.  It works
with every particle model and both draws, inside the particle kernels: no further pass on the device.

`wind=(wx, wz)` (default (0, 0): off) is the air's mean horizontal velocity in m/s, x right and z toward the viewer in the particle
world's axes (the camera for 'iid' and 'field', the rig for 'rig', the world under a trajectory; tools/particles.py wind=,
`main.py --wind WX,WZ`): rain in a 5 m/s cross-wind falls at 40 degrees to the vertical, small drops leaning more than large ones.
`lean=None` (default) follows the wind: with a non-zero wind the renderer takes a streak tile's lean and corner from the streak
itself (RR_OPT_STREAK_LEAN), without one it keeps the reference's rule; True / False force either.

`gusts=GustSeries` (default None: off; 'field' and 'rig' only) is a wind that changes over time: the air's horizontal displacement
sampled at the frame indices frame0 .. frame0 + n (tools/particles.py gust_series makes one; `main.py --gusts SIGMA[,TAU[,SEED]]`;
DESIGN 5k).  `frame_index` then also selects the wind: a clip k0 + arange(T) sways coherently, random indices into a long series give
every image of a batch its own slant.  A frame_index outside the series is a ValueError.  `lean=None` is on with a series too.
`set_gusts()` takes another series between batches.

`showers=RateSeries` (default None: off; 'field' and 'rig' only) is a rain rate that changes over time: mm/hr sampled at the frame
indices frame0 .. frame0 + n (tools/particles.py RateSeries; shower_series makes one that builds, peaks and fades;
`main.py --showers LOW,PERIOD_S[,PHASE]`).  The slots, tables and `drops_cap` are those of the series' peak and never
change; `frame_index` then also selects the rate: a clip k0 + arange(T) shows ONE field whose drops thin out and come back -- a
drop that has started to fall keeps falling -- and image i's fog constants are those of the rate at frame_index[i].  `intensity`
is then None or the series' peak (anything else is a ValueError, as is None without a series), and a frame_index outside the
series is a ValueError.  `set_showers()` takes another series between batches.

`lens=LensDrops` (default None: off; tools/lens.py) puts adherent drops on the camera's lens: after the rain, the rainy
images go through the lens pass (rr_lens_drops_device: one more kernel, k_lens_drops) on the same stream.  Each drop is a small
inverted, minified, defocused view of the rainy image with a soft edge and a dark rim, and sits still for seconds: `frame_index[i]`
selects the table, `lens.table(frame_index[i])`; under the rig model view v wears `lens.for_view(views[v])`.  The LensDrops' H, W
must be the augmenter's frame size (ValueError).  The streak mask comes back unchanged; `return_lens_alpha=True` returns a third
tensor, float32 [B, 1, H, W] ([B, V, 1, H, W] for a rig): the drops' coverage, 0 outside them -- the label raindrop-removal work trains
on.  `LensAugment(lens)` is the lens pass alone, for drops without streak rain: `(images, frame_index) -> images`.

`source_size=(Hs, Ws)` (default None: the images have the render size `frame_size()`) takes full-size frames when the dataset renders
at a fraction of its files' resolution (Cityscapes: render_scale 2): `images` is [B, 3, Hs, Ws] ([B, V, 3, Hs, Ws] under a rig) and
the library resizes it on the device with the frame loader's own interpolation (rr_set_input_resize; csrc/rr_resize.h)
before anything else.  `depth_size=(Hd, Wd)` (default None: the render size) is the size of `depth`, resized the same way.  `rainy`,
`mask`, the lens pass and `return_lens_alpha` stay at the render size.  The contract: uint8 images of the source size give the RGB of
the PNG a `main.py --device_particles` run at that render scale writes for files holding those pixels (and a depth file holding
depth * 256); float32 images are widened, not re-quantised to bytes, so they match that run to the image contract only (+-1 LSB) --
the mask is identical either way.  Shapes that do not match, or a `depth_size` other than the render size without `source_size`,
are a ValueError.

`return_layer=True` (default False) returns one thing more, last: a `RainLayer`, the streaks of every image without the
image -- what de-raining, rain-removal and rain-segmentation models train on beside the rainy frame and the rain-free target.
`.colour` [B, 3, H, W] (L) and `.transmittance` [B, 1, H, W] (T) are float32 views of one tensor, `.background` [B, 3, H, W] is the
fogged image the streaks were composited over (the rain-free target; the float32 values the compositor read) and `.shift` [B] the
frame's mean shift (float64, on the device); `.over(x)` is clamp(T x + L - shift, 0, 1), which for x = `.background` gives `rainy`
to the byte's last place wherever no blend saturated.  Always planar float32 at the render size, whatever the images' dtype and
layout; under a rig the tensors gain the V axis the images have; with `lens=` the layer is that of the streaks alone (the lens pass
comes after it, as for the mask).  It costs one more kernel over the compositor's work lists (k_rain_layer), no second render.

One library call per batch (rr_augment_frames_device: particles, planar ingest, fog + environment-map pre-pass, hot path, planar
finalize) on the caller's current stream; it returns once the batch is complete.  The set-up -- camera, simulation options, fog
constants, particle tables, environment-map geometry and solid angles -- comes from the functions the driver uses.  Not offered:
the 'white' strategy and opacity attenuation.  The reference's `--noise_std` depends on the order of a run, which random access
does not have: `jitter` is the per-drop tilt that random access, moving particles and shared views can have.

This module imports torch; the package's __init__ does not."""
import numbers
import os

import numpy as np
import torch

from . import hip_backend
from .common import add_attenuation, envmap, imgops, solid_angle
from .common import db as dbmod
from .common.bad_weather import DBManager
from . import rig as rigmod
from .trajectory import Trajectory
from .tools import lens as lensmod
from .tools import particles


def sim_options(dataset, sequence=None):
    """The particle simulation options of `sequence` (common.db.sim, what main.py --device_particles hands the generator); with
    no sequence the dataset's own settings, without any sequence-specific entry."""
    if sequence is not None:
        return dbmod.sim(dataset, sequence, '')['options']
    opts = dict(dbmod.settings(dataset))
    opts.pop('sequences', None)
    return opts


def _as_list(v, B, name, kind):
    """A number (one value for every image) or B values, as a list of Python numbers."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    if isinstance(v, numbers.Number) or (isinstance(v, np.ndarray) and v.ndim == 0):
        vals = [v.item() if isinstance(v, np.ndarray) else v] * B
    else:
        try:
            vals = list(np.asarray(v).reshape(-1).tolist())
        except Exception:
            raise TypeError("%s must be a number or a sequence of %d numbers" % (name, B))
        if len(vals) != B:
            raise ValueError("%s: %d values for a batch of %d images" % (name, len(vals), B))
    for x in vals:
        if isinstance(x, bool) or not isinstance(x, numbers.Number):
            raise TypeError("%s must hold numbers, got %r" % (name, x))
        if kind == 'index' and x != int(x):
            raise TypeError("%s must hold integers, got %r" % (name, x))
    return vals


_DTYPES = {torch.uint8: hip_backend.RR_TENSOR_U8, torch.float32: hip_backend.RR_TENSOR_F32,
           torch.float16: hip_backend.RR_TENSOR_F16, torch.bfloat16: hip_backend.RR_TENSOR_BF16}
LENS_FORMATS = "uint8 batches (planar or channels-last) and planar float32 batches"


def tensor_layout(images):
    """How the frames [..., 3, H, W] of `images` lie in memory: 'planar' (contiguous), 'interleaved' (a dense NHWC view: channel
    stride 1, W stride 3, H stride 3 W, the leading dims packed) or None (anything else: the caller makes it planar-contiguous).
    The stride of a dim of size 1 says nothing and is not looked at."""
    if images.is_contiguous():
        return 'planar'
    shape, stride = tuple(images.shape), tuple(images.stride())
    H, W = shape[-2], shape[-1]
    want = {-3: 1, -1: 3, -2: 3 * W}
    step = 3 * H * W
    for d in range(-4, -len(shape) - 1, -1):
        want[d] = step
        step *= shape[d]
    if all(shape[d] == 1 or stride[d] == v for d, v in want.items()):
        return 'interleaved'
    return None


def _empty_like_frames(shape, dtype, device, layout):
    """An uninitialised [..., 3, H, W] tensor in `layout`."""
    if layout != 'interleaved':
        return torch.empty(shape, dtype=dtype, device=device)
    lead, (H, W) = tuple(shape[:-3]), shape[-2:]
    nd = len(lead)
    return torch.empty(lead + (H, W, 3), dtype=dtype, device=device).permute(*range(nd), nd + 2, nd, nd + 1)


class RainLayer:
    """The streaks of a batch as colour and transmittance (RainAugment(return_layer=True); the contract: csrc/rr_layer.h).
    colour [.., 3, H, W] and transmittance [.., 1, H, W] are views of the one float32 tensor [.., 4, H, W] (R, G, B, T) the library
    wrote; background [.., 3, H, W] float32; shift [..] float64.  All on the images' device, planar, at the render size."""

    def __init__(self, planes, background, shift):
        self.planes, self.background, self.shift = planes, background, shift
        self.colour = planes.narrow(-3, 0, 3)
        self.transmittance = planes.narrow(-3, 3, 1)

    def over(self, x):
        """clamp(T x + L - shift, 0, 1) for x [.., 3, H, W] with values in [0, 1] (bytes: x / 255 first), evaluated in float64;
        float32 out (float64 for a float64 x).  over(background) is the rainy image before its truncation to bytes."""
        if not isinstance(x, torch.Tensor) or not x.is_floating_point() or x.shape != self.background.shape:
            raise ValueError("x must be a floating-point tensor of shape %s" % (tuple(self.background.shape),))
        v = self.transmittance.double() * x.double() + self.colour.double() - self.shift[..., None, None, None]
        return v.clamp_(0.0, 1.0).to(torch.float64 if x.dtype == torch.float64 else torch.float32)


class RainAugment:
    """Callable: (images, depth, intensity, frame_index) -> (rainy, mask[, lens alpha][, RainLayer]).  See the module docstring."""

    def __init__(self, dataset='kitti', streaks_db='3rdparty/rainstreakdb', sequence=None, device=None, seed=0, particle_model='iid',
                 rig=None, views=None, draws='stream', jitter=0.0, trajectory=None, wind=(0.0, 0.0), lean=None, gusts=None, showers=None,
                 lens=None, return_lens_alpha=False, source_size=None, depth_size=None, return_layer=False):
        if not isinstance(return_layer, bool):
            raise ValueError("return_layer=%r: True or False" % (return_layer,))
        self.return_layer = return_layer
        if lens is not None and not isinstance(lens, lensmod.LensDrops):
            raise TypeError("lens must be a tools.lens.LensDrops, got %r" % (type(lens).__name__,))
        if not isinstance(return_lens_alpha, bool) or (return_lens_alpha and lens is None):
            raise ValueError("return_lens_alpha=%r: True or False, and True needs lens=" % (return_lens_alpha,))
        self.lens, self.return_lens_alpha = lens, return_lens_alpha
        self._lens_views = {}                    # view number -> lens.for_view(view)
        if particle_model not in particles.MODELS:
            raise ValueError("particle_model %r: expected one of %s" % (particle_model, ', '.join(particles.MODELS)))
        self.particle_model = particle_model
        if draws not in particles.DRAWS:
            raise ValueError("draws %r: expected one of %s" % (draws, ', '.join(particles.DRAWS)))
        self.draws = draws
        if isinstance(jitter, bool) or not isinstance(jitter, numbers.Number) or not np.isfinite(jitter) or jitter < 0:
            raise ValueError("jitter %r: expected a finite number of degrees >= 0" % (jitter,))
        self.jitter = float(jitter)
        try:
            if isinstance(wind, (str, bytes)) or len(wind) != 2 or any(isinstance(v, bool) or not isinstance(v, numbers.Number) for v in wind):
                raise TypeError
            self.wind = particles._check_wind(wind)
        except TypeError:
            raise ValueError("wind %r: expected two numbers (wx, wz) in m/s" % (wind,))
        if lean is not None and not isinstance(lean, bool):
            raise ValueError("lean %r: expected None (follow the wind), True or False" % (lean,))
        self._lean_arg = lean
        if (particle_model == 'rig') != (rig is not None):
            raise ValueError("particle_model='rig' and rig= go together (rig.Rig)")
        if rig is None and views is not None:
            raise ValueError("views= selects views of a rig: it needs particle_model='rig'")
        self.rig, self.views = rig, None
        if rig is not None:
            if not isinstance(rig, rigmod.Rig):
                raise TypeError("rig must be a rig.Rig, got %r" % (type(rig).__name__,))
            self.views = rigmod.check_active(views, len(rig))
        self.dataset, self.sequence, self.seed = dataset, sequence, int(seed)
        st = dbmod.settings(dataset)
        self.settings = st
        self.options = sim_options(dataset, sequence)
        self.render_scale = int(st['render_scale'])
        self.focal = st['cam_focal'] / 1000.
        self.f_number, self.exposure, self.camera_gain = st['cam_f_number'], st['cam_exposure'], st['cam_gain']
        self.n_sim = particles.n_sim_frames(self.options)
        self.trajectory = self._check_trajectory(trajectory)
        self.gusts = particles._check_gusts(gusts, self.options["cam_hz"], particle_model)
        self.lean = bool(self.wind[0] or self.wind[1] or self.gusts is not None) if lean is None else lean
        self.showers = particles._check_rate_series(showers, particle_model)
        light_db = os.path.join(streaks_db, 'env_light_database')
        self.db = DBManager(streaks_path=os.path.join(light_db, 'size32'),
                            norm_coeff_path=os.path.join(light_db, 'txt', 'normalized_env_max.txt'))
        self.db.load_streak_database()
        if device is not None:
            device = torch.device(device) if not isinstance(device, int) else torch.device('cuda', device)
            if device.type != 'cuda':
                raise ValueError("RainAugment renders on a GPU: device must be a CUDA (HIP) device, got %s" % device)
            if device.index is None:
                device = torch.device('cuda', torch.cuda.current_device())
        self.device = device                     # None: the current device at the first call
        self._hip = None
        self._rates = {}                         # intensity -> (sims, cdf tables, fog constants)
        self._unions = {}                        # sorted intensities -> (d_grid, cdf of all their tables, table offset per intensity)
        self._tables_key = None                  # the union the context holds
        self._geom = None                        # (H, W) whose envmap geometry and solid angles the context holds
        self._traj_set = trajectory is None      # whether the context holds the current trajectory's box and table
        self._gusts_set = gusts is None          # whether the context holds the current gust series
        self._showers_set = showers is None      # whether the context holds the current rate series
        self._fogs = {}                          # rate -> fog constants (a rate series: one rate per frame index)
        if lens is not None and (lens.H, lens.W) != self.frame_size():
            raise ValueError("lens: the LensDrops are for %d x %d frames (H x W), %s renders %d x %d" %
                             ((lens.H, lens.W, dataset) + self.frame_size()))
        self.source_size, self.depth_size = self._check_sizes(source_size, depth_size)
        self._resize_set = self.source_size is None          # whether the context holds the input sizes

    def _check_sizes(self, source_size, depth_size):
        """(source_size, depth_size) as pairs of ints, or (None, None): the images and depth maps have the render size."""
        def pair(v, name):
            if v is None:
                return None
            try:
                a, b = v
                ok = all(not isinstance(x, bool) and isinstance(x, numbers.Integral) and 1 <= x <= 16384 for x in (a, b))
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("%s %r: expected (H, W), integers in [1, 16384]" % (name, v))
            return int(a), int(b)
        source_size, depth_size = pair(source_size, 'source_size'), pair(depth_size, 'depth_size')
        if source_size is None:
            if depth_size is not None and depth_size != self.frame_size():
                raise ValueError("depth_size %r differs from the render size %r: it needs source_size= (the stage that resizes both)" %
                                 (depth_size, self.frame_size()))
            return None, None
        return source_size, depth_size if depth_size is not None else self.frame_size()

    def _check_trajectory(self, trajectory):
        if trajectory is None:
            return None
        if self.rig is None:
            raise ValueError("trajectory= needs particle_model='rig' (a single camera: rig=Rig.from_spec('mono'))")
        if not isinstance(trajectory, Trajectory):
            raise TypeError("trajectory must be a trajectory.Trajectory, got %r" % (type(trajectory).__name__,))
        return trajectory.at_rate(self.options["cam_hz"])    # frame_index counts frames of the run: row f is t = f / cam_hz

    def set_trajectory(self, trajectory):
        """Another trajectory (or None: the rig stands still) from the next call on: between batches, with no call in flight.  The
        slot counts and tables follow its box, so frames made under different trajectories share no drops."""
        self.trajectory = self._check_trajectory(trajectory)
        self._rates, self._unions, self._tables_key = {}, {}, None
        self._traj_set = False

    def set_gusts(self, gusts):
        """Another gust series (or None: the mean wind alone) from the next call on: between batches, with no call in flight.  With
        lean=None the renderer's lean follows: on with a series or a non-zero wind."""
        self.gusts = particles._check_gusts(gusts, self.options["cam_hz"], self.particle_model)
        if self._lean_arg is None:
            self.lean = bool(self.wind[0] or self.wind[1] or self.gusts is not None)
        self._gusts_set = False

    def set_showers(self, showers):
        """Another rate series (or None: one intensity per image again) from the next call on: between batches, with no call in
        flight.  The slots and tables follow the series' peak."""
        self.showers = particles._check_rate_series(showers, self.particle_model)
        self._showers_set = False

    # ---- host side: what a call sends (no GPU needed) ----------------------------------------------------------------
    def frame_size(self):
        """(H, W) of the frames this dataset's simulation renders (sensor size / render_scale)."""
        sims = self._rate(self._first_rate())[0]
        return int(sims[0]['sensor_h']) // self.render_scale, int(sims[0]['sensor_w']) // self.render_scale

    def _first_rate(self):
        if self.showers is not None and not self._rates:
            return self.showers.peak
        return next(iter(self._rates)) if self._rates else 25.0

    def _fog(self, rate):
        """FogRain.constants at `rate` mm/hr (a rate series: image i's rate is the series' at frame_index[i])."""
        rate = float(rate)
        if rate not in self._fogs:
            fog = add_attenuation.FogRain(rain_intensity=rate, focal=self.focal, f_number=self.f_number, angle=90,
                                          exposure=self.exposure, camera_gain=self.camera_gain).constants()
            self._fogs[rate] = tuple(float(v) for v in fog)
        return self._fogs[rate]

    def _rate(self, rate):
        """The driver's run set-up at one intensity (common/generator.py: sim_frames at seed `seed`, FogRain.constants)."""
        rate = float(rate)
        if rate not in self._rates:
            sims, dgrid, cdf = particles.sim_frames(self.options, rate, self.n_sim, render_scale=self.render_scale, seed=self.seed,
                                                    model=self.particle_model, rig=self.rig, trajectory=self.trajectory)
            fog = add_attenuation.FogRain(rain_intensity=rate, focal=self.focal, f_number=self.f_number, angle=90,
                                          exposure=self.exposure, camera_gain=self.camera_gain).constants()
            self._rates[rate] = (sims, dgrid, np.atleast_2d(cdf), tuple(float(v) for v in fog))
        return self._rates[rate]

    def _union(self, rates):
        key = tuple(sorted(set(float(r) for r in rates)))
        if key not in self._unions:
            tabs, offs, dgrid = [], {}, None
            for r in key:
                _, dg, cdf, _ = self._rate(r)
                assert dgrid is None or np.array_equal(dgrid, dg), "diameter grids of one context must agree"
                dgrid = dg
                offs[r] = sum(len(t) for t in tabs)
                tabs.append(cdf)
            self._unions[key] = (dgrid, np.ascontiguousarray(np.concatenate(tabs)), offs)
        return key, self._unions[key]

    def plan(self, intensity, frame_index, B=None):
        """What a call sends for these intensities and frame indices: dict(sims = SIM_FRAME_DTYPE records, d_grid, cdf = the
        union of the intensities' diameter tables the records index, fog = [B, 4] pre-pass constants, drops_cap, key, particle_model,
        cam_hz, draws, jitter, wind, gusts, showers (expected_records' rate_series): what expected_records needs; lean: the renderer's RR_OPT_STREAK_LEAN to state the call's drop tables).  Under the
        rig model B counts instants: sims and fog hold V = len(views) consecutive entries per instant (view views[i % V] of
        instant i // V), plus views, rig_views and rig_box (what rr_set_particle_rig gets)."""
        if B is None:
            B = len(np.atleast_1d(np.asarray(frame_index.cpu() if isinstance(frame_index, torch.Tensor) else frame_index)))
        idx = [int(f) for f in _as_list(frame_index, B, 'frame_index', 'index')]
        if self.showers is not None:                         # the series says the rate; the slots and tables are its peak's
            peak = self.showers.peak
            if intensity is not None and any(float(r) != peak for r in _as_list(intensity, B, 'intensity', 'rate')):
                raise ValueError("intensity %r: with showers= the rate comes from the series; pass None or its peak %r" % (intensity, peak))
            rates = [peak] * B
        elif intensity is None:
            raise ValueError("intensity=None needs showers= (a rate series)")
        else:
            rates = [float(r) for r in _as_list(intensity, B, 'intensity', 'rate')]
        if any(not (r > 0) or not np.isfinite(r) for r in rates):
            raise ValueError("intensity must be positive (mm/hr), got %r" % (rates,))
        if any(f < 0 or f >= 2 ** 32 for f in idx):
            raise ValueError("frame_index must hold integers in [0, 2^32), got %r" % (idx,))
        if self.gusts is not None and not self.gusts.covers(idx).all():
            raise ValueError("frame_index %r is outside the gust series' frames %d .. %d" % (
                [f for f in idx if not self.gusts.covers(f)], self.gusts.frame0, self.gusts.frame0 + self.gusts.n - 1))
        if self.showers is not None and not self.showers.covers(idx).all():
            raise ValueError("frame_index %r is outside the rate series' frames %d .. %d" % (
                [f for f in idx if not self.showers.covers(f)], self.showers.frame0, self.showers.frame0 + self.showers.n - 1))
        key, (dgrid, cdf, offs) = self._union(rates)
        sims = np.zeros(B, hip_backend.SIM_FRAME_DTYPE)
        fog = np.zeros((B, 4), np.float64)
        n_max = 0
        for i, (r, f) in enumerate(zip(rates, idx)):
            rs, _, _, fc = self._rate(r)
            sims[i] = rs[f % self.n_sim]                     # simulated frame f % n_sim with the draws of frame f (generator.py:318-321)
            sims[i]['draw_seed'] = f
            if self.particle_model in ('field', 'rig'):      # the field's time is the frame index itself: a clip is k0 + arange(T)
                sims[i]['frame'] = f
            sims[i]['table'] = int(rs[f % self.n_sim]['table']) + offs[r]
            sims[i]['run_pos'] = 0
            fog[i] = fc if self.showers is None else self._fog(self.showers.rate_at(f))
        for r in key:
            n_max = max(n_max, int(self._rate(r)[0]['n_particles'].max()))
        # the driver's capacity of a frame's drop table (generator.py _run_batches_native + _Slot)
        drops_cap = (min(max(1024, n_max), 2 ** 16) + 3) // 4 * 4
        out = dict(sims=sims, d_grid=dgrid, cdf=cdf, fog=fog, drops_cap=min(drops_cap, 2 ** 16), key=key, frame_size=self.frame_size(),
                   source_size=self.source_size, depth_size=self.depth_size,     # (None, None: images and depth at the render size)
                   particle_model=self.particle_model, cam_hz=float(self.options["cam_hz"]), draws=self.draws, jitter=self.jitter,
                   wind=self.wind, lean=self.lean, gusts=self.gusts, showers=self.showers)
        if self.rig is not None:                             # V consecutive records per instant, equal up to draw_seed (equal too)
            V = len(self.views)
            box_rig = self.rig if self.trajectory is None else self.trajectory.bind(self.rig)
            out.update(sims=np.repeat(sims, V), fog=np.repeat(fog, V, axis=0), views=list(self.views),
                       rig_views=self.rig.as_records(), rig_box=particles.rig_run_box(self.options, self._first_rate(), self.n_sim, box_rig))
            if self.trajectory is not None:                  # frame_index selects the pose
                if any(f >= len(self.trajectory) for f in idx):
                    raise ValueError("frame_index %r is outside the trajectory's %d poses" % ([f for f in idx if f >= len(self.trajectory)],
                                                                                              len(self.trajectory)))
                if len(set(sims['exposure_s'].tolist())) != 1:
                    raise ValueError("a trajectory needs one exposure for the whole batch")
                out.update(trajectory=self.trajectory, traj_poses=self.trajectory.compose(self.rig, float(sims[0]['exposure_s'])))
        return out

    # ---- the call ----------------------------------------------------------------------------------------------------
    def _validate(self, images, depth):
        if not isinstance(images, torch.Tensor) or not isinstance(depth, torch.Tensor):
            raise TypeError("images and depth must be torch tensors")
        if images.dtype not in _DTYPES:
            raise TypeError("images must be uint8 or float32 (or float16 / bfloat16), got %s" % images.dtype)
        if self.rig is not None:
            V = len(self.views)
            if images.dim() != 5 or images.shape[1] != V or images.shape[2] != 3 or min(images.shape) < 1:
                raise ValueError("images must be [B, V = %d, 3, H, W] (RGB per view; the shape, whatever the strides), got %s" % (V, tuple(images.shape)))
            B, _, _, H, W = images.shape
            dH, dW = (H, W) if self.source_size is None else self.depth_size
            if depth.dtype != torch.float32 or tuple(depth.shape) not in ((B, V, dH, dW), (B, V, 1, dH, dW)):
                raise ValueError("depth must be float32 [B, V, H, W] or [B, V, 1, H, W] = %s, got %s %s" %
                                 ((B, V, dH, dW), depth.dtype, tuple(depth.shape)))
            return B, H, W
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1 or images.shape[2] < 1 or images.shape[3] < 1:
            raise ValueError("images must be [B, 3, H, W] (RGB; the shape, whatever the strides), got %s" % (tuple(images.shape),))
        B, _, H, W = images.shape
        dH, dW = (H, W) if self.source_size is None else self.depth_size
        if depth.dtype != torch.float32 or tuple(depth.shape) not in ((B, dH, dW), (B, 1, dH, dW)):
            raise ValueError("depth must be float32 [B, H, W] or [B, 1, H, W] = %s, got %s %s" % ((B, dH, dW), depth.dtype, tuple(depth.shape)))
        return B, H, W

    def _layout(self, images):
        """The layout the call reads `images` in: 'interleaved' for a dense NHWC view, else 'planar' (contiguous, or made so).  With
        lens=, a format the lens pass does not take is a ValueError here, before any GPU work."""
        layout = tensor_layout(images) or 'planar'
        if self.lens is not None and (images.dtype in (torch.float16, torch.bfloat16) or
                                      (images.dtype == torch.float32 and layout == 'interleaved')):
            raise ValueError("lens= takes %s, got a %s %s batch" % (LENS_FORMATS, layout, images.dtype))
        return layout

    def _check_device(self, images, depth):
        for name, t in (('images', images), ('depth', depth)):
            if t.device.type != 'cuda':
                raise ValueError("%s must be on the GPU (a CUDA / HIP tensor), got a %s tensor" % (name, t.device.type))
        dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        for name, t in (('images', images), ('depth', depth)):
            if t.device != dev:
                raise ValueError("%s is on %s, the augmenter's context on %s" % (name, t.device, dev))
        return dev

    def _context(self, dev, H, W, key, dgrid, cdf, p=None):
        if self._hip is None:
            hip = hip_backend.RainHip(dev.index)
            hip.set_streak_db(self.db.streaks_light)
            hip.set_camera(hip_backend.make_camera(self.focal, self.f_number, self.exposure))
            hip.set_prepass_kernels(imgops.gaussian_kernel(25, 25), imgops.gaussian_kernel(15, 0))
            if self.rig is not None:
                hip.set_particle_rig(p['rig_views'], p['rig_box'], active=p['views'])
            hip.set_particle_model(self.particle_model, self.options["cam_hz"])
            hip.set_particle_draws(self.draws)
            hip.set_particle_jitter(self.jitter)
            hip.set_particle_wind(*self.wind)
            hip.set_option(hip_backend.RR_OPT_STREAK_LEAN, int(self.lean))
            self._hip, self.device = hip, dev
        if self.rig is not None and not self._traj_set:      # (the previous call has finished: no kernel reads the old table)
            self._hip.set_particle_rig(p['rig_views'], p['rig_box'], active=p['views'])      # the box is the trajectory's
            self._hip.set_particle_trajectory(p.get('traj_poses'))
            self._traj_set = True
        if not self._gusts_set:                  # (the previous call has finished: no kernel reads the old series)
            self._hip.set_particle_gusts(self.gusts)
            self._hip.set_option(hip_backend.RR_OPT_STREAK_LEAN, int(self.lean))
            self._gusts_set = True
        if not self._showers_set:                # (likewise)
            self._hip.set_particle_rate_series(self.showers)
            self._showers_set = True
        if self._tables_key != key:              # (the previous call has finished: no kernel reads the old tables)
            self._hip.set_particle_tables(dgrid, cdf)
            self._tables_key = key
        if self._geom != (H, W):                 # envmap geometry + resident solid angles, per frame size
            we = self._hip.set_envmap_geometry(H, W, *envmap.EnvironmentMapGenerator(self.focal, W, H).device_tables(H, W))
            self._hip.set_solid_angles(solid_angle.get_solid_angles(np.empty((H, we, 0))))
            self._geom = (H, W)
        if not self._resize_set:                 # full-size frames in: the library resizes images and depth to H x W first
            self._hip.set_input_resize(*(self.source_size + self.depth_size))
            self._resize_set = True
        return self._hip

    def __call__(self, images, depth, intensity, frame_index):
        B, H, W = self._validate(images, depth)
        layout = self._layout(images)
        p = self.plan(intensity, frame_index, B)
        fh, fw = int(p['sims'][0]['sensor_h']) // self.render_scale, int(p['sims'][0]['sensor_w']) // self.render_scale
        if (H, W) != ((fh, fw) if self.source_size is None else self.source_size):
            raise ValueError("%s%s renders %d x %d frames (H x W)%s, the images are %d x %d" %
                             (self.dataset, '' if self.sequence is None else '/' + self.sequence, fh, fw,
                              '' if self.source_size is None else ' from source_size = %d x %d' % self.source_size, H, W))
        dev = self._check_device(images, depth)
        V = None if self.rig is None else len(self.views)
        if V is not None:                                    # the library's batch: V consecutive frames per instant
            B = B * V
        if layout == 'planar':                               # (an interleaved batch is read where it lies: B frames of [H, W, 3])
            images = images.reshape(B, 3, H, W).contiguous()
        depth = depth.reshape((B,) + ((H, W) if self.source_size is None else self.depth_size)).contiguous()
        H, W = fh, fw                                        # from here on: the render size
        with torch.cuda.device(dev):
            hip = self._context(dev, H, W, p['key'], p['d_grid'], p['cdf'], p)
            rainy = _empty_like_frames((B, 3, H, W), images.dtype, dev, layout)
            mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
            sims = np.ascontiguousarray(p['sims'])
            fog = np.ascontiguousarray(p['fog'])
            b = hip_backend.rr_tensor_batch()
            b.n, b.H, b.W = B, H, W
            b.dtype = _DTYPES[images.dtype]
            b.layout = hip_backend.RR_LAYOUT_INTERLEAVED if layout == 'interleaved' else hip_backend.RR_LAYOUT_PLANAR
            b.images, b.depth = images.data_ptr(), depth.data_ptr()
            b.sims, b.fog = sims.ctypes.data, fog.ctypes.data
            b.drops_cap = p['drops_cap']
            b.rainy_out, b.mask_out = rainy.data_ptr(), mask.data_ptr()
            stream = torch.cuda.current_stream(dev)
            if not stream.cuda_stream:
                # the legacy default stream is handle 0, which the library reads as "the context's own stream": what torch has
                # queued on it (the inputs) is finished first, and the call's own wait covers the outputs
                stream.synchronize()
            layer = None
            if self.return_layer:                # three more tensors for the call to fill: planar float32 / float64, the render size
                layer = RainLayer(torch.empty((B, 4, H, W), dtype=torch.float32, device=dev),
                                  torch.empty((B, 3, H, W), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float64, device=dev))
                hip.augment_set_layer(layer.planes.data_ptr(), layer.background.data_ptr(), layer.shift.data_ptr())
            try:
                hip.augment_frames_device(b, stream.cuda_stream)
            finally:
                if layer is not None:
                    hip.augment_set_layer()
            alpha = None
            if self.lens is not None:            # the drops on the lens refract the rainy image: one more kernel on the same stream
                idx = [int(f) for f in _as_list(frame_index, B if V is None else B // V, 'frame_index', 'index')]
                rainy, alpha = _lens_pass(hip, self._lens_tables(idx), self.lens.weights(), rainy, self.return_lens_alpha, stream,
                                          'hwc' if layout == 'interleaved' else 'chw')
        if V is not None:
            rainy, mask = rainy.unflatten(0, (B // V, V)), mask.reshape(B // V, V, 1, H, W)      # (a view in either layout)
            alpha = None if alpha is None else alpha.reshape(B // V, V, 1, H, W)
            if layer is not None:
                layer = RainLayer(layer.planes.reshape(B // V, V, 4, H, W), layer.background.reshape(B // V, V, 3, H, W), layer.shift.reshape(B // V, V))
        out = (rainy, mask, alpha) if self.return_lens_alpha else (rainy, mask)
        return out + (layer,) if self.return_layer else out

    def _lens_tables(self, idx):
        """The drop tables of a call, one per image of the library's batch: frame_index[i]'s; under a rig, V per instant, view v's own."""
        if self.rig is None:
            return [self.lens.table(f) for f in idx]
        for v in self.views:
            if v not in self._lens_views:
                self._lens_views[v] = self.lens.for_view(v)
        return [self._lens_views[v].table(f) for f in idx for v in self.views]

    def close(self):
        if self._hip is not None:
            self._hip.close()
            self._hip = None


def _lens_pass(hip, tables, weights, images, want_alpha, stream, layout='chw'):
    """rr_lens_drops_device on the [n, 3, H, W] tensor `images` -- contiguous, or with layout='hwc' uint8 in a dense NHWC view -- on
    `stream`: (images with the drops, in the same layout, alpha or None)."""
    n, _, H, W = images.shape
    out = _empty_like_frames(images.shape, images.dtype, images.device, 'interleaved' if layout == 'hwc' else 'planar')
    alpha = torch.empty((n, 1, H, W), dtype=torch.float32, device=images.device) if want_alpha else None
    hip.lens_drops_device(images.data_ptr(), out.data_ptr(), n, H, W, images.dtype == torch.float32, tables, weights,
                          alpha_ptr=None if alpha is None else alpha.data_ptr(), stream=stream.cuda_stream, layout=layout)
    return out, alpha


class LensAugment:
    """Callable: (images, frame_index) -> images with the drops of `lens` (tools/lens.py LensDrops) on them -- the lens pass of
    RainAugment(lens=) alone, for drops without streak rain.  `images` is [B, 3, H, W] on the GPU, uint8 or float32, H x W the
    LensDrops' (a uint8 channels-last batch is read where it lies and comes back channels-last; any other striding is made planar first);
    image i wears `lens.table(frame_index[i])`.  return_alpha=True: (images, alpha), alpha float32 [B, 1, H, W], the
    drops' coverage.  Enqueued on the caller's current stream; on the legacy default stream the call waits for the result."""

    def __init__(self, lens, device=None, return_alpha=False):
        if not isinstance(lens, lensmod.LensDrops):
            raise TypeError("lens must be a tools.lens.LensDrops, got %r" % (type(lens).__name__,))
        self.lens, self.return_alpha = lens, bool(return_alpha)
        if device is not None:
            device = torch.device(device) if not isinstance(device, int) else torch.device('cuda', device)
            if device.type != 'cuda':
                raise ValueError("LensAugment renders on a GPU: device must be a CUDA (HIP) device, got %s" % device)
            if device.index is None:
                device = torch.device('cuda', torch.cuda.current_device())
        self.device = device                     # None: the current device at the first call
        self._hip = None

    def __call__(self, images, frame_index):
        if not isinstance(images, torch.Tensor):
            raise TypeError("images must be a torch tensor")
        if images.dtype not in (torch.uint8, torch.float32):
            raise TypeError("images must be uint8 or float32, got %s" % images.dtype)
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError("images must be [B, 3, H, W] (the shape, whatever the strides), got %s" % (tuple(images.shape),))
        B, _, H, W = images.shape
        if (H, W) != (self.lens.H, self.lens.W):
            raise ValueError("the LensDrops are for %d x %d frames (H x W), the images are %d x %d" % (self.lens.H, self.lens.W, H, W))
        idx = [int(f) for f in _as_list(frame_index, B, 'frame_index', 'index')]
        if any(f < 0 for f in idx):
            raise ValueError("frame_index must hold integers >= 0, got %r" % (idx,))
        if images.device.type != 'cuda':
            raise ValueError("images must be on the GPU (a CUDA / HIP tensor), got a %s tensor" % images.device.type)
        dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        if images.device != dev:
            raise ValueError("images is on %s, the augmenter's context on %s" % (images.device, dev))
        tables = [self.lens.table(f) for f in idx]
        with torch.cuda.device(dev):
            if self._hip is None:
                self._hip, self.device = hip_backend.RainHip(dev.index), dev
            stream = torch.cuda.current_stream(dev)
            if not stream.cuda_stream:           # handle 0 is "the context's own stream" to the library: finish the inputs first
                stream.synchronize()
            if images.dtype == torch.uint8 and tensor_layout(images) == 'interleaved':
                out, alpha = _lens_pass(self._hip, tables, self.lens.weights(), images, self.return_alpha, stream, 'hwc')
            else:
                out, alpha = _lens_pass(self._hip, tables, self.lens.weights(), images.contiguous(), self.return_alpha, stream)
        return (out, alpha) if self.return_alpha else out

    def close(self):
        if self._hip is not None:
            self._hip.close()
            self._hip = None
