"""Rain-particle generator: the stand-in for the reference's external simulator, on the host AND on the device.

The reference drives a closed-source binary (``3rdparty/weather-particle-simulator/.../AHLSimulation``) through
``tools/simulation.py`` / ``tools/particles_simulation.py`` with the settings of ``common/db.py:41-70``
(``cam_hz``, ``cam_CCD_WH``, ``cam_CCD_pixsize``, ``cam_focal``, ``cam_exposure``, ``sim_mode``, ``sim_steps``
{``cam_motion``, ``cam_exposure``, ``cam_focal``, ``rain_fallrate``}, ``sim_duration``) and reads its output back as
``<particles>/<dataset>/<sequence>/rain/<N>mm/*_camera0.xml`` (schema: bad_weather.py:192-211).  There is no source
for that binary, so there is nothing to compare against bit for bit: this is a physically motivated generator, validated
statistically (tests/test_particles.py), that takes the SAME settings and emits the SAME schema.

The model is stated twice, with identical bits:
  * HERE, in numpy (``generate``): the product's host path -- it writes the XML file the reference's loader reads when a
    simulation is missing (``simulate``, main.py) -- and the definition the device is tested against;
  * in ``csrc/rr_particles.h`` (``k_particles`` in rainhip.hip): BASELINE.json configs[4], "in-kernel particle simulation
    (no XML)": the library generates the particles, applies the loader's derived fields and the frame filter, makes the
    renderer's per-drop random draws and leaves ``rr_drop[]`` records in HBM (``rr_generate_drops_device``, or
    ``rr_frame_in.sim`` in the host-pointer entry points).  ``sim_frames`` / ``diameter_tables`` below describe a run to
    the library; ``expected_records`` is what it must produce (tests/test_gpu_particles.py: bit for bit).
Arithmetic shared by both: IEEE double with the evaluation order spelled out, + - * / sqrt rint floor only (exp through
``det_exp``: the same operations on every machine), random numbers from the counter-based Philox4x32-10 -- particle i of
frame k is a pure function of (seed, k, i), so any lane of any GPU can make it.

Model (per camera frame, camera at the origin looking along -z, x right, y up, image origin bottom-left -- the
conventions the loader undoes, bad_weather.py:221-224):
  * drop diameters follow Marshall & Palmer (1948): N(D) = N0 exp(-Lambda D), N0 = 8000 m^-3 mm^-1,
    Lambda = 4.1 R^-0.21 mm^-1 for a fall rate R in mm/hr, D in [0.5, 6] mm;
  * only drops that can appear at least `min_px` wide are simulated: depth z <= D f / (pixel * min_px) (and <= z_far),
    uniformly in the viewing frustum up to that depth -- the expected count is the integral of N(D) over that volume,
    the actual count of a frame is Poisson distributed (drawn by the host: one number per frame);
  * a drop falls at its terminal velocity v(D) = 9.65 - 10.3 exp(-0.6 D) m/s (Atlas et al. 1973), drifts with a
    horizontal wind (bell-shaped: a centred sum of four uniforms scaled to `wind_sigma`) and approaches the camera at the
    vehicle's speed (``sim_steps['cam_motion']``, km/h); the streak is the path covered during the exposure, both ends
    projected through the pinhole camera;
  * image widths are D f / (pixel z) at either end.

Two particle models share all of the above.  The default, i.i.d. model (``model='iid'``) draws a fresh, independent set of
particles for every simulated frame.  The FIELD model (``model='field'``, ``make_field_particles``; ``rr_set_particle_model``
in the library) is a persistent, stateless particle field for video:
  * a run has a fixed number of particle SLOTS, drawn once per distinct settings of the run (``field_slot_counts``: Poisson
    around three times the expected count, because a slot lives in the axis-aligned box that bounds its frustum and a
    pyramid fills a third of its bounding box).  Slot j has a diameter D_j (same table, same ``sample_diameter``, hence the
    same z_max(D) cut) and a phase for good: Philox block (j, 0, 0, 1);
  * the box of a slot has half sides bx = hx z_max, by = hy z_max (hx, hy: the margin-enlarged frustum's half-widths at unit
    depth) and depth 0 .. z_max.  The slot falls through it once every T = 2 by / v(D) seconds.  At time t = k / cam_hz the
    number of completed falls is g = floor(t / T + phase) (the slot's LIFE) and the fractional part its age.  A life's own
    draws (lateral start, start depth, wind) come from blocks (j, g mod 2^32, 1 | 2, 2 + g / 2^32): every life of a slot
    is a new drop, nothing recurs;
  * inside a life the position is the start moved by velocity x elapsed time: v(D) down, the life's wind sideways, the
    vehicle's speed towards the camera; the two lateral axes wrap modulo the box.  A translation modulo the box keeps a
    uniform law uniform, so at every single t the particles inside the frustum (the others are culled, two slots in
    three) are uniform by volume up to z_max(D) with the i.i.d. model's expected count: the two models are equal in law
    frame by frame, and differ in that frame k + 1 of the field shows frame k's drops a little lower and closer;
  * the streak of a frame is the path covered during the exposure from the position at t_k, both ends projected;
  * the TIME is the rendered frame's index f itself (it does not wrap); the SETTINGS of frame f are those of simulated frame
    f % n_sim.  Motion is continuous across frames whose settings agree; where the settings of two consecutive frames
    differ (``sim_mode == "steps"``: speed, focal length, exposure or fall rate per step) the boxes, periods and tables
    differ and the field may jump (a fall rate that changes WITHOUT a jump is a rate series: Showers, below);
  * particle (slot j, frame k) is a pure function of (seed, j, k) and the settings: any frame can be made alone, in any
    batch, on any rank, with the same bits.  The kept records of a frame are in ascending slot order.  Angular noise
    (``--noise_std``) is not defined for the field model.

The RIG model (``model='rig'``, ``make_rig_particles``; ``rr_set_particle_rig``) is the field model in the frame of a camera
rig: one lattice world (a slot's box wraps in x and z), each view p_cam = R (p_rig - c) looks at the lattice image nearest to
its camera (rig.py).

A TRAJECTORY (``trajectory=``, ``make_rig_particles(view_end=)``; ``rr_set_particle_trajectory``, trajectory.py) moves and turns
the rig through that unchanged world.  Every (time index k, view) has two world -> camera poses, composed with the rig's views
on the host: (R0, c0) at t_k and (R1, c1) at t_k + exposure.  The view step, in this order:
    d = (X, Y, Z) - c0; dx, dz wrapped to the nearest image; (xc, yc, zc) = R0 d; cull        -- the rig model's, word for word
    e = (d + (wind, -v, speed_mps) exposure) - (c1 - c0)                                         -- the camera's own displacement
    (X2, Y2, Z2) = R1 e                                            -- the same lattice image as the start, never wrapped again
and everything downstream (projection, the loader's fields, bucket, pick, jitter) is unchanged.  With R1 == R0 and c1 == c0 the
subtraction is - 0.0: the rig model's bits for the view (R0, c0).  speed_mps remains a drift of the world; ``sim_frames`` writes
0 under a trajectory, because the trajectory says how the camera moves.  The slot counts and tables take ``Trajectory.box``: the
reach of all headings and the altitude range.  The rotation during the exposure is taken at its two ends only.

Per-drop draws (``draws=``, ``rr_set_particle_draws`` in the library).  ``'stream'`` (default) is the renderer's own: numpy's
legacy stream seeded per frame picks one of the ten textures of the drop's ratio bucket (``randint(lo, lo + 10)``), in
drop order -- what a run that writes the reference's files needs.  ``'counter'`` (``counter_picks``) takes the pick from
the drop's own Philox counter instead: ``pick = (w * 10) >> 32`` with w = word 2 of the drop's block 1 -- (i, frame, 1, 0),
or the life's block (j, g_lo, 1, 2 + g_hi) under the field and rig models; a word the generator computes anyway and no
other draw reads -- and ``tex_index = 10 * texture_bucket(ratio) + pick``.  Under the field and rig models the pick is a
function of (seed, slot, life): a drop keeps its texture in every frame of its life and in every view of the rig (the
ratio BUCKET comes from the projected size and can still differ between frames or views).  Under the i.i.d. model it is a
function of (seed, frame, particle index).  ``draw_seed`` is ignored.  Angular noise needs the stream's normal deviates
and run order and is refused with counter draws.

Streak jitter (``jitter=DEG``, ``rr_set_particle_jitter`` in the library; ``counter_jitter``).  Every drop has a standard normal
deviate g of its own: Box-Muller on its Philox block 3 -- (i, frame, 3, 0), or the life's block (j, g_lo, 3, 2 + g_hi) under the
field and rig models; the generators read blocks 0 .. 2 (and (j, 0, 0, 1) for a slot), nothing else reads block 3.  After
the loader's derived fields and the frame filter, every kept non-Big streak is turned by ``jitter * g`` degrees the way the
angular noise turns one (``noise_rotation``: rotation terms by the angle sum, end points about the midpoint, truncated).  The
kept set, sizes, texture and world positions do not depend on it.  Under the field and rig models g is a function of
(seed, slot, life): a drop keeps its tilt in every frame of its life and in every view.  It is not ``--noise_std`` (whose
deviates come from the run's sequential stream) and is refused together with it.

Mean wind (``wind=(wx, wz)``, ``rr_set_particle_wind`` in the library): the air's mean horizontal velocity in m/s, in the axes
of the particle world -- x right, z toward the viewer: the camera frame of the i.i.d. and field models, the rig frame of the
rig model, the lattice's world frame under a trajectory.  ``_drift`` adds it to a drop's horizontal velocity once,
``vx = wind_life + wx`` and ``vz = speed + wz``, and those two take the place of the life's wind and of the speed wherever they
enter: the end of the streak in every model, and the position inside a life of the field and rig models (a translation modulo
the box: the law at one instant does not change).  Slot counts, boxes, lives and tables do not depend on it.  ``(0, 0)``
(default) is off and forms no sum at all (``x + 0.0`` is not ``x`` for ``x = -0.0``, which ``_block_wind`` gives at
``wind_sigma = 0``): the records are those without the keyword, byte for byte.  A uniform slant needs the renderer's
``RR_OPT_STREAK_LEAN``.  The host XML writer's default path (``simulate``) has no wind.

Gusts (``gusts=GustSeries``, ``rr_set_particle_gusts`` in the library; field and rig models): a wind that changes over time, as
the air's horizontal DISPLACEMENT sampled at frame times.  ``disp[(n + 1), 2]`` holds (x, z) metres, row i at time index
``frame0 + i``; the air moves linearly between samples.  The table is data: the host makes it any way it likes
(``gust_series``: an Ornstein-Uhlenbeck velocity), the statements only look up, interpolate and add (``_gust_terms``).  With
m = frame - frame0 (0 <= m < n) and back = tau cam_hz the frames since the life's birth:
    sb = m - back;  i = max(floor(sb), 0);  Gb = G[i] + (sb - i) (G[i + 1] - G[i])     -- the air at the drop's birth
    dG = G[m] - Gb                                                  -- the air's displacement over the drop's life so far
    ge = (G[m + 1] - G[m]) cam_hz                                   -- the air's velocity during this frame's interval
(before the series starts the first interval's velocity is held: a constant-velocity series is a mean wind).  They enter where
the mean wind enters: ``(vx tau + dGx) / box`` in the position of a life, ``vx + gex`` in the streak's end (the rig slot's
velocity carries it: every view and a trajectory's end pose use it unchanged); vx, vz are ``_drift``'s, and with a series both
mean-wind additions are formed, also for a mean of (0, 0).  Nothing else depends on the series: slot counts, boxes, lives,
Philox blocks, tables, the pick, the jitter.  Inside a life the term is a translation modulo the box that does not depend on the
uniform start: one frame keeps the i.i.d. law.  Drops follow the air with no inertia.  ``gusts=None`` (default) is off and forms
no addition.  The i.i.d. model has no time and refuses a series.

Showers (``rate_series=RateSeries``, ``rr_set_particle_rate_series`` in the library; field and rig models): a rain rate that
changes over time.  ``rate[n + 1]`` holds mm/hr, row i at time index ``frame0 + i``.  The run's slots, slot counts, boxes and
tables are those of the series' PEAK rate and never change; a life of a slot is kept with the probability
``N(D; R) / N(D; R_peak) = exp(-(Lambda(R) - Lambda(R_peak)) D)`` (at most 1 for R <= R_peak) of the rate R at the life's BIRTH
time: the peak's field thinned to the field at rate R, in law, and a drop that has started to fall keeps falling.  The host turns
the series into the table ``L[i] = min(mp_lambda(rate[i]) - mp_lambda(peak), RATE_DLAM_MAX)`` (``RateSeries.dlam``; a rate of 0
gives RATE_DLAM_MAX), the statements look up, interpolate and compare (``_rate_alive``).  With m = frame - frame0 (0 <= m < n):
    sb = max(m - tau cam_hz, 0);  i = floor(sb);  Lb = L[i] + (sb - i) (L[i + 1] - L[i])   -- Lambda's excess at the drop's birth
    p = det_exp(-(Lb D));  alive = unit32(b[3]) < p                        -- b[3]: word 3 of the life's block 1, read by nothing else
(before the series starts its first value is held -- no extrapolation).  A life that is not alive is culled exactly as a slot
outside the frustum is; under the rig model the decision belongs to the slot (``rig_state``), so every view and a trajectory
agree.  Lb = 0 gives p = 1.0 exactly: a series that sits at its peak gives the records of no series, byte for byte.  Lb = 100
gives p < 2^-33, the smallest ``unit32``: a rate of 0 admits no new drop.  Nothing else depends on the series: slot counts, boxes,
lives, periods, tables, positions, the pick, the jitter, wind and gusts.  So where the rate changes during a clip the field no
longer jumps.  The rate seen at time t is the rate at the drops' birth times: large near drops lag by up to one fall period.
``rate_series=None`` (default) is off and forms none of the above.  The i.i.d. model has no time and refuses a series.
"""
import os

import numpy as np

from ..common.bad_weather import PARTICLE_DTYPE, PARTICLE_FRAME_DTYPE

N0 = 8000.0                      # m^-3 mm^-1
D_MIN, D_MAX = 0.5, 6.0          # mm
N_GRID = 512                     # entries of the diameter table


def mp_lambda(fallrate):
    """Marshall-Palmer slope, mm^-1."""
    return 4.1 * float(fallrate) ** -0.21


def det_exp(x):
    """exp(x) for -700 < x <= 0 from + - * / (and an exact power of two) only: identical bits in numpy, g++ and on gfx950
    (csrc/rr_device.h det_exp is the same sequence of operations)."""
    x = np.asarray(x, np.float64)
    k = np.rint(x * 1.44269504088896338700e+00)
    r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
    p = np.full_like(r, 1.0 / 6227020800.0)
    for c in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0):
        p = p * r + 1.0 / c
    p = p * r + 1.0
    p = p * r + 1.0
    return np.ldexp(p, k.astype(np.int64))


# ---- angular noise (--noise_std) on device-generated tables: the same statement in rr_device.h / rr_particles.h ---------
# log and sin / cos in the style of det_exp: + - * / sqrt rint and exact power-of-two scaling only, so that numpy, g++ and
# gfx950 agree to the bit.  Polynomials of fdlibm / musl (public domain): within an ulp of the exact value.
_LG = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
       1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)
_LN2_HI, _LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
      -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_C = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
      2.08757232129817482790e-09, -1.13596475577881948265e-11)
_INV_PIO2, _PIO2_1, _PIO2_2, _PIO2_2T = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050630396597660e-11, \
    2.02226624879595063154e-21
DEG2RAD = np.pi / 180                                     # np.deg2rad(x) is x * (pi / 180)


def det_log(x):
    """log(x) for 0 < x < 1 (the polar method's r2): x = m 2^e by frexp (exact), m in [sqrt(1/2), sqrt(2)), then fdlibm's
    log1p polynomial in s = f / (2 + f), f = m - 1 (exact).  rr_device.h det_log is the same sequence of operations."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    lo = m < 0.70710678118654752440
    m = np.where(lo, m * 2.0, m)
    k = (e - lo).astype(np.float64)
    f = m - 1.0
    hfsq = 0.5 * f * f
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (_LG[1] + w * (_LG[3] + w * _LG[5]))
    t2 = z * (_LG[0] + w * (_LG[2] + w * (_LG[4] + w * _LG[6])))
    r = t2 + t1
    return k * _LN2_HI - ((hfsq - (s * (hfsq + r) + k * _LN2_LO)) - f)


def det_sincos(x):
    """(sin x, cos x): Cody-Waite reduction by pi/2 in three parts (k pi/2 exact for |k| < 2^20, i.e. |x| < 1.6e6, some
    9e7 degrees), then musl's kernels on [-pi/4, pi/4].  Same bits everywhere for any finite x; NaN for inf / NaN."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid='ignore'):
        return _det_sincos(x)


def _det_sincos(x):
    k = np.rint(x * _INV_PIO2)
    r = ((x - k * _PIO2_1) - k * _PIO2_2) - k * _PIO2_2T
    z = r * r
    w = z * z
    rs = (_S[1] + z * (_S[2] + z * _S[3])) + (z * w) * (_S[4] + z * _S[5])
    sr = r + (z * r) * (_S[0] + z * rs)
    rc = z * (_C[0] + z * (_C[1] + z * _C[2])) + (w * w) * (_C[3] + z * (_C[4] + z * _C[5]))
    hz = 0.5 * z
    wc = 1.0 - hz
    cr = wc + (((1.0 - wc) - hz) + z * rc)
    q = k - 4.0 * np.rint(k * 0.25)                       # quadrant in {-2 .. 2}, exact (0 beyond 2^53)
    qi = np.where(np.isfinite(q), q, 0).astype(np.int64) & 3
    sn = np.select([qi == 0, qi == 1, qi == 2], [sr, cr, -sr], -cr)
    cn = np.select([qi == 0, qi == 1, qi == 2], [cr, -sr, -cr], sr)
    return sn, cn


def polar_factor(r2):
    """numpy's legacy_gauss: the polar pair (x1, x2) with r2 = x1^2 + x2^2 in (0, 1) gives f * x2 now and f * x1 next."""
    return np.sqrt(-2.0 * det_log(r2) / r2)


def legacy_draws(seed, tex_lo, is_big):
    """One frame's drop loop for np.random.seed(seed): per drop randint(lo, lo + 10), per non-Big drop the legacy normal
    deviate (0 for Big drops) -- numpy's stream word for word, the deviate with det_log instead of libm's log."""
    rs = np.random.RandomState(int(seed))
    words, at = [], [0]

    def u32():
        if at[0] == len(words):
            words.extend(rs.randint(0, 2 ** 32, size=4096, dtype=np.uint32).tolist())
        at[0] += 1
        return words[at[0] - 1]

    def dbl():
        a, b = u32() >> 5, u32() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0
    n = len(tex_lo)
    tex = np.zeros(n, np.int32)
    g = np.zeros(n, np.float64)
    cached = None
    for i, (lo, big) in enumerate(zip(np.asarray(tex_lo).tolist(), np.asarray(is_big).tolist())):
        v = u32() & 15
        while v > 9:
            v = u32() & 15
        tex[i] = lo + v
        if big:
            continue
        if cached is not None:
            g[i], cached = cached, None
            continue
        while True:
            x1, x2 = 2.0 * dbl() - 1.0, 2.0 * dbl() - 1.0
            r2 = x1 * x1 + x2 * x2
            if r2 < 1.0 and r2 != 0.0:
                break
        f = float(polar_factor(r2))
        cached = f * x1
        g[i] = f * x2
    return tex, g


def noise_degrees(g, noise_std, noise_scale):
    """normal(0, noise_std) * noise_scale in the reference's operation order (generator.py:136)."""
    return (0.0 + noise_std * np.asarray(g, np.float64)) * noise_scale


def noise_rotation(s, e, noise_deg):
    """Rotation terms and rotated end points of streaks (start / end: (n, 2) integer positions) turned by noise_deg:
    rot_cos / rot_sin = cos / sin(-(theta + noise) * pi / 180) (generator.py:138-163) as the angle sum of the exact
    cos / sin(-theta) = -dy / n, -|dx| / n and det_sincos(noise); the end points turned about their midpoint in
    hip_backend.pack_frame's operation order and truncated toward zero like numpy's int64 store."""
    s = np.asarray(s).astype(np.float64)
    e = np.asarray(e).astype(np.float64)
    sn, cn = det_sincos(np.asarray(noise_deg, np.float64) * DEG2RAD)
    with np.errstate(all='ignore'):
        d = s - e
        n1 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        c0 = (d[:, 0] / n1) * 0.0 + (d[:, 1] / n1) * -1.0
        s0 = -(np.abs(d[:, 0]) / n1)
        rot_cos = c0 * cn + s0 * sn
        rot_sin = s0 * cn - c0 * sn
    mx = (e[:, 0] + s[:, 0]) / 2
    my = (e[:, 1] + s[:, 1]) / 2
    s2 = np.stack([(s[:, 0] - mx) * cn - (s[:, 1] - my) * sn + mx, (s[:, 0] - mx) * sn + (s[:, 1] - my) * cn + my], axis=1).astype(np.int64)
    e2 = np.stack([(e[:, 0] - mx) * cn - (e[:, 1] - my) * sn + mx, (e[:, 0] - mx) * sn + (e[:, 1] - my) * cn + my], axis=1).astype(np.int64)
    return rot_cos, rot_sin, s2, e2


def noise_step(table, imW, imH, ratio_db, seed, noise_std, noise_scale):
    """One frame of a run with angular noise on a StreakTable, in place: the frame filter on the current end points, the
    frame's draws over the kept streaks, the rotation of the kept non-Big ones.  Returns the frame's DROP_DTYPE records
    (rotation terms from the end points before the step, end points after it) -- what the device's chain step makes."""
    from .. import hip_backend
    idx = hip_backend.filter_streaks(table, imW, imH)
    out = np.zeros(len(idx), hip_backend.DROP_DTYPE)
    if len(idx) == 0:
        return out
    r = table.ratio[idx]
    b = np.full(len(idx), 4, np.int32)
    for k in (3, 2, 1, 0):                                # take_drop_texture's blocks of ten (NaN: the last one)
        b = np.where(r < ratio_db[k], k, b)
    types = table.type[idx]
    tex, g = legacy_draws(seed, 10 * b, types == 0)
    nb = types != 0
    rot_cos, rot_sin, s2, e2 = noise_rotation(table.ips[idx], table.ipe[idx], noise_degrees(g, noise_std, noise_scale))
    table.ips[idx[nb]] = s2[nb]
    table.ipe[idx[nb]] = e2[nb]
    out['x0'], out['y0'] = table.ips[idx, 0], table.ips[idx, 1]
    out['x1'], out['y1'] = table.ipe[idx, 0], table.ipe[idx, 1]
    out['max_width'], out['length'], out['type'], out['tex_index'] = table.max_width[idx], table.length[idx], types, tex
    out['iw1'], out['iw2'], out['wps'], out['wpe'] = table.iw1[idx], table.iw2[idx], table.wps[idx], table.wpe[idx]
    out['rot_cos'] = np.where(nb, rot_cos, 1.0)
    out['rot_sin'] = np.where(nb, rot_sin, 0.0)
    return out


def terminal_velocity(d_mm):
    """m/s (Atlas, Srivastava & Sekhon 1973)."""
    return 9.65 - 10.3 * det_exp(-0.6 * np.asarray(d_mm, np.float64))


# ---- Philox4x32-10 (Salmon, Moraes, Dror & Shaw, SC'11) ---------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, key0, key1):
    """Four uint32 words per counter (c0..c3 broadcast against each other); the key is two 32-bit integers."""
    c = [np.asarray(v, np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(key0) & 0xFFFFFFFF, int(key1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def unit32(w):
    """A 32-bit word as a number strictly inside (0, 1): (w + 1/2) / 2^32, exact in double."""
    return (np.asarray(w, np.float64) + 0.5) * (1.0 / 4294967296.0)


class FrameCamera:
    def __init__(self, options, step):
        """The camera of simulation step `step`: `options` is what common.db.sim() returns under "options"."""
        steps = options.get("sim_steps", {}) or {}

        def stepped(key, default):
            v = steps.get(key)
            if v is None or len(v) == 0:
                return default
            return float(v[min(step, len(v) - 1)])           # a parameter stays applied unless later changed (db.py)
        self.W, self.H = (int(v) for v in options["cam_CCD_WH"])
        self.pix = options["cam_CCD_pixsize"] * 1e-6
        self.focal = stepped("cam_focal", options["cam_focal"]) * 1e-3
        self.exposure = stepped("cam_exposure", options["cam_exposure"]) * 1e-3
        self.speed = stepped("cam_motion", 0.0) / 3.6         # km/h -> m/s
        self.fpx = self.focal / self.pix
        self.hz = options["cam_hz"]


def _diameter_cdf(dens, d):
    """(total, sampling CDF) of a density `dens` (drops per mm of diameter) on the grid `d`: trapezoid rule."""
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(d))])
    total = float(cdf[-1])
    cdf = cdf / cdf[-1]
    cdf[-1] = 1.0
    return total, cdf


def expected_count(cam, fallrate, min_px=1.0, z_far=15.0, margin=0.05, n_grid=N_GRID):
    """(expected visible drops per frame, diameter grid, its sampling CDF, z_max per diameter)."""
    d = np.linspace(D_MIN, D_MAX, n_grid)
    z_max = np.minimum(d * 1e-3 * cam.fpx / min_px, z_far)
    area = (1 + 2 * margin) ** 2 * cam.W * cam.H / cam.fpx ** 2          # frustum cross-section at unit depth
    total, cdf = _diameter_cdf(N0 * det_exp(-mp_lambda(fallrate) * d) * area * z_max ** 3 / 3.0, d)
    return total, d, cdf, z_max


def sample_diameter(dgrid, cdf, u):
    """Inverse-CDF sample: the last j with cdf[j] <= u, linear inside the cell (rr_particles.h sample_diameter)."""
    j = np.minimum(np.searchsorted(cdf, u, side='right') - 1, len(cdf) - 2)
    slope = (dgrid[j + 1] - dgrid[j]) / (cdf[j + 1] - cdf[j])
    return dgrid[j] + (u - cdf[j]) * slope


def _frame_settings(options, fallrate, k, min_px, z_far, margin):
    steps = options.get("sim_steps", {}) or {}
    cam = FrameCamera(options, k)
    rates = steps.get("rain_fallrate", ())
    rate = float(rates[min(k, len(rates) - 1)]) if len(rates) else float(fallrate)
    return cam, rate


MODELS = ('iid', 'field', 'rig')


DRAWS = ('stream', 'counter')


def _check_draws(draws, noisy=False):
    if draws not in DRAWS:
        raise ValueError("particle draws %r: expected one of %s" % (draws, ', '.join(DRAWS)))
    if draws == 'counter' and noisy:
        raise ValueError("counter draws have no angular noise: the noise needs the stream's normal deviates and run order")


def texture_pick(w):
    """rr_particles.h texture_pick: a 32-bit word scaled to 0 .. 9, (w * 10) >> 32 in 64-bit."""
    return ((np.asarray(w).astype(np.uint64) * np.uint64(10)) >> np.uint64(32)).astype(np.int64)


def _life_counter(j, life, block):
    """rr_particles.h life_counter: the counter (j, g mod 2^32, block, 2 + g / 2^32) of block `block` of the slots' lives g."""
    g = np.asarray(life, np.float64)
    g_hi = np.floor(g * (1.0 / 4294967296.0))
    g_lo = g - g_hi * 4294967296.0
    return j, g_lo.astype(np.uint64), block, np.uint64(2) + g_hi.astype(np.uint64)


def _drop_block(seed, pid, block, frame, life):
    """Philox block `block` of the drops `pid`: (pid, frame, block, 0) of the i.i.d. model, or the life's (_life_counter)."""
    j = np.asarray(pid).astype(np.uint64)
    counter = (j, int(frame) & 0xFFFFFFFF, block, 0) if life is None else _life_counter(j, life, block)
    return philox4x32(*counter, *_key(seed))


def counter_picks(seed, pid, frame=None, life=None):
    """The counter-based texture pick (0 .. 9) of particles `pid`: texture_pick of word 2 of the drop's Philox block 1.
    i.i.d. model: `frame` = the simulated frame, block (pid, frame, 1, 0).  Field and rig models: `life` = the life g of every
    slot `pid` (make_field_particles / make_rig_particles return it), block (pid, g_lo, 1, 2 + g_hi)."""
    return texture_pick(_drop_block(seed, pid, 1, frame, life)[2])


def jitter_deviate(w0, w1, w2):
    """rr_particles.h jitter_deviate: a standard normal deviate from three 32-bit words by Box-Muller.  u1 has 53 bits in
    (0, 1] (every step exact), u2 = unit32(w2); g = sqrt(-2 det_log(u1)) * cos(2 pi u2) with det_log / det_sincos: + - * / sqrt
    only, the same bits in numpy, g++ and on gfx950.  |g| <= sqrt(2 * 53 * ln 2) < 8.6; u1 = 1 gives 0."""
    a = (np.asarray(w0).astype(np.uint64) >> np.uint64(5)).astype(np.float64)
    b = (np.asarray(w1).astype(np.uint64) >> np.uint64(6)).astype(np.float64)
    u1 = ((a * 67108864.0 + b) + 1.0) * (1.0 / 9007199254740992.0)
    _, cn = det_sincos(6.283185307179586 * unit32(w2))
    return np.sqrt(-2.0 * det_log(u1)) * cn


def counter_jitter(seed, pid, frame=None, life=None):
    """The streak-jitter deviate (standard normal) of particles `pid`: jitter_deviate of the drop's Philox block 3, which no
    other draw reads.  i.i.d. model: `frame` = the simulated frame, block (pid, frame, 3, 0).  Field and rig models: `life` = the
    life g of every slot `pid`, block (pid, g_lo, 3, 2 + g_hi) -- laid out like the life's blocks 1 and 2."""
    w = _drop_block(seed, pid, 3, frame, life)
    return jitter_deviate(w[0], w[1], w[2])


def _check_jitter(jitter, noisy=False, run=None):
    jitter = float(jitter)
    if not np.isfinite(jitter) or jitter < 0:
        raise ValueError("streak jitter %r: expected a finite number of degrees >= 0" % jitter)
    if jitter and (noisy or run is not None):
        raise ValueError("streak jitter cannot be combined with angular noise (noise_std / noise_scale / run): the jitter is a "
                         "function of the drop, the noise of the run's order")
    return jitter


def jitter_records(rec, g, jitter):
    """Turn the kept non-Big records of one frame (DROP_DTYPE, in place) by jitter * g degrees: rr_particles.h noise_rotate on
    each.  `g`: the deviate of every record.  Big records are left alone; a streak of zero length gets NaN rotation terms."""
    nb = rec['type'] != 0
    if not nb.any():
        return rec
    s = np.stack([rec['x0'], rec['y0']], axis=1)
    e = np.stack([rec['x1'], rec['y1']], axis=1)
    rot_cos, rot_sin, s2, e2 = noise_rotation(s, e, float(jitter) * np.asarray(g, np.float64))
    rec['rot_cos'][nb], rec['rot_sin'][nb] = rot_cos[nb], rot_sin[nb]
    rec['x0'][nb], rec['y0'][nb] = s2[nb, 0], s2[nb, 1]
    rec['x1'][nb], rec['y1'][nb] = e2[nb, 0], e2[nb, 1]
    return rec


def _check_model(model):
    if model not in MODELS:
        raise ValueError("particle model %r: expected one of %s" % (model, ', '.join(MODELS)))


def _key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def frame_counts(options, fallrate, n_frames, seed=0, min_px=1.0, z_far=15.0, margin=0.05, count=None):
    """Particles simulated per frame: Poisson around the model's mean (legacy RandomState: one draw per frame, by the
    host), or `count` for every frame (benchmarks with fixed drop counts)."""
    out = np.zeros(n_frames, np.int64)
    for k in range(n_frames):
        if count is not None:
            out[k] = int(count)
            continue
        cam, rate = _frame_settings(options, fallrate, k, min_px, z_far, margin)
        mean = expected_count(cam, rate, min_px, z_far, margin)[0]
        out[k] = int(np.random.RandomState((int(seed) * 1000003 + k) % (2 ** 32)).poisson(mean))
    return out


def _slot_z_max(cam, wd, min_px, z_far):
    """rr_particles.h slot_z_max: only drops that can show at least min_px wide are simulated (wd: the diameter in metres)."""
    return np.minimum((wd * cam.fpx) / min_px, z_far)


def _block_wind(c, wind_sigma):
    """rr_particles.h block_wind: a centred sum of the block's four uniforms scaled to unit variance, times wind_sigma."""
    s4 = ((unit32(c[0]) + unit32(c[1])) + (unit32(c[2]) + unit32(c[3]))) - 2.0
    return (s4 * 1.7320508075688772) * wind_sigma


def _check_wind(wind):
    """(wx, wz) as two floats; rr_set_particle_wind's refusals."""
    try:
        wx, wz = (float(v) for v in wind)
    except (TypeError, ValueError):
        raise ValueError("mean wind %r: expected two numbers (wx, wz) in m/s" % (wind,))
    if not (np.isfinite(wx) and np.isfinite(wz)) or abs(wx) > 100.0 or abs(wz) > 100.0:
        raise ValueError("mean wind %r: each component is a finite number of m/s of magnitude <= 100" % (wind,))
    return wx, wz


def _drift(wind_life, speed, wind, gusts=None):
    """A drop's horizontal velocity (vx, vz) under the mean wind `wind` (rr_particles.h WIND): the life's own wind plus wx, the
    vehicle's speed plus wz -- one addition each.  wind == (0, 0): the two inputs themselves, no addition (module docstring) --
    unless a gust series is given: the gust path forms both additions whatever the mean."""
    wx, wz = _check_wind(wind)
    if wx == 0.0 and wz == 0.0 and gusts is None:
        return wind_life, speed
    return wind_life + wx, float(speed) + wz


# ---- gusts: the air's displacement sampled at frame times (module docstring; rr_set_particle_gusts) -------------------
GUST_MAX_N = 1 << 20                 # intervals of a series
GUST_MAX_DISP = 1e6                  # metres
GUST_MAX_SPEED = 100.0               # m/s over any interval


class GustSeries:
    """frame0: the time index of row 0; disp [(n + 1), 2]: the air's horizontal displacement (x, z) in metres at time indices
    frame0 .. frame0 + n.  Covers the frames frame0 <= k < frame0 + n."""

    def __init__(self, frame0, disp):
        self.frame0 = int(frame0)
        self.disp = np.ascontiguousarray(disp, np.float64)

    @property
    def n(self):
        return len(self.disp) - 1

    def covers(self, k):
        k = np.asarray(k, np.int64)
        return (k >= self.frame0) & (k < self.frame0 + self.n)


def _check_gusts(gusts, cam_hz, model='field', frames=None):
    """rr_set_particle_gusts' refusals (and the generator's, for the time indices `frames`) as ValueError.  Returns `gusts`."""
    if gusts is None:
        return None
    if not isinstance(gusts, GustSeries):
        raise ValueError("gusts %r: expected a particles.GustSeries or None" % (gusts,))
    if model not in ('field', 'rig'):
        raise ValueError("a gust series needs particle model 'field' or 'rig': the i.i.d. model has no time")
    if cam_hz is None or not np.isfinite(float(cam_hz)) or not float(cam_hz) > 0:
        raise ValueError("a gust series needs cam_hz > 0")
    G = gusts.disp
    if G.ndim != 2 or G.shape[1] != 2 or len(G) < 2:
        raise ValueError("gust series: disp must be (n + 1) x 2 with n >= 1, got shape %r" % (G.shape,))
    n = len(G) - 1
    if n > GUST_MAX_N:
        raise ValueError("gust series: n = %d is beyond 2^20 intervals" % n)
    if gusts.frame0 < 0 or gusts.frame0 + n > 2 ** 32:
        raise ValueError("gust series: frame0 %d + n %d must lie in 0 .. 2^32" % (gusts.frame0, n))
    if not np.isfinite(G).all():
        raise ValueError("gust series: every displacement must be finite")
    if (np.sqrt(G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) > GUST_MAX_DISP).any():
        raise ValueError("gust series: a displacement is beyond 1e6 m")
    st = G[1:] - G[:-1]
    if (np.sqrt(st[:, 0] * st[:, 0] + st[:, 1] * st[:, 1]) * float(cam_hz) > GUST_MAX_SPEED).any():
        raise ValueError("gust series: an interval's |step| * cam_hz is beyond 100 m/s")
    if frames is not None and not gusts.covers(np.asarray(frames, np.int64) & 0xFFFFFFFF).all():
        raise ValueError("time index outside the gust series' frames %d .. %d" % (gusts.frame0, gusts.frame0 + n - 1))
    return gusts


def gust_series(n, cam_hz, sigma, tau_s, seed, frame0=0):
    """A GustSeries of n intervals at cam_hz frames per second: per component an Ornstein-Uhlenbeck velocity with stationary
    standard deviation `sigma` (m/s) and correlation time `tau_s` (seconds), one value per interval (exact discretisation:
    u[i + 1] = a u[i] + sigma sqrt(1 - a^2) N(0, 1), a = exp(-1 / (cam_hz tau_s)), u[0] = sigma N(0, 1)), from
    np.random.RandomState(seed).  The displacement is the sequential sum of velocity / cam_hz from 0 (np.add.accumulate)."""
    n, cam_hz, sigma, tau_s = int(n), float(cam_hz), float(sigma), float(tau_s)
    if n < 1 or n > GUST_MAX_N:
        raise ValueError("gust_series: n must be 1 .. 2^20, got %d" % n)
    if not (np.isfinite(cam_hz) and cam_hz > 0 and np.isfinite(sigma) and sigma >= 0 and np.isfinite(tau_s) and tau_s > 0):
        raise ValueError("gust_series: cam_hz > 0, sigma >= 0 and tau_s > 0 must be finite")
    rs = np.random.RandomState(int(seed) % (2 ** 32))
    z = rs.standard_normal((n, 2))
    a = float(np.exp(-1.0 / (cam_hz * tau_s)))
    b = sigma * float(np.sqrt(1.0 - a * a))
    u = np.zeros((n, 2), np.float64)
    u[0] = sigma * z[0]
    for i in range(1, n):
        u[i] = a * u[i - 1] + b * z[i]
    disp = np.zeros((n + 1, 2), np.float64)
    disp[1:] = np.add.accumulate(u / cam_hz, axis=0)
    return _check_gusts(GustSeries(frame0, disp), cam_hz)


def _gust_terms(gusts, k, tau, cam_hz):
    """rr_particles.h gust_birth / gust_terms: (dG (n, 2), ge (2,)) of the slots whose lives began `tau` seconds before time
    index k (module docstring): look up, interpolate, add -- one operation per step."""
    G = gusts.disp
    m = (int(k) & 0xFFFFFFFF) - gusts.frame0
    if not 0 <= m < gusts.n:
        raise ValueError("time index %d is outside the gust series' frames %d .. %d" % (int(k), gusts.frame0, gusts.frame0 + gusts.n - 1))
    back = tau * float(cam_hz)
    sb = float(m) - back
    i = np.maximum(np.floor(sb), 0.0)
    ii = i.astype(np.int64)
    fr = sb - i
    g0, g1 = G[ii], G[ii + 1]
    Gb = g0 + fr[:, None] * (g1 - g0)
    dG = G[m][None, :] - Gb
    ge = (G[m + 1] - G[m]) * float(cam_hz)
    return dG, ge


# ---- showers: the rain rate sampled at frame times (module docstring; rr_set_particle_rate_series) -------------------
RATE_MAX_N = 1 << 20                 # intervals of a series
RATE_DLAM_MAX = 100.0                # mm^-1: det_exp(-(100 D)) is below every unit32 for D >= 0.5 mm


class RateSeries:
    """frame0: the time index of row 0; rate [n + 1]: the rain rate in mm/hr at time indices frame0 .. frame0 + n; peak: the
    rate the run's slots and tables are drawn for (default: max(rate)).  Covers the frames frame0 <= k < frame0 + n."""

    def __init__(self, frame0, rate, peak=None):
        self.frame0 = int(frame0)
        self.rate = np.ascontiguousarray(rate, np.float64)
        self._peak = None if peak is None else float(peak)

    @property
    def n(self):
        return len(self.rate) - 1

    @property
    def peak(self):
        return float(self.rate.max()) if self._peak is None else self._peak

    def covers(self, k):
        k = np.asarray(k, np.int64)
        return (k >= self.frame0) & (k < self.frame0 + self.n)

    def rate_at(self, k):
        """The rate at time index k (frame0 <= k <= frame0 + n)."""
        return float(self.rate[int(k) - self.frame0])

    def dlam(self):
        """rr_set_particle_rate_series' table: L[i] = min(mp_lambda(rate[i]) - mp_lambda(peak), RATE_DLAM_MAX), [n + 1] mm^-1."""
        lp = mp_lambda(self.peak)
        return np.asarray([min(mp_lambda(r) - lp, RATE_DLAM_MAX) if r > 0.0 else RATE_DLAM_MAX for r in self.rate.tolist()], np.float64)


def _check_rate_series(rate_series, model='field', frames=None):
    """rr_set_particle_rate_series' refusals (and the generator's, for the time indices `frames`) as ValueError.  Returns
    `rate_series`."""
    if rate_series is None:
        return None
    if not isinstance(rate_series, RateSeries):
        raise ValueError("rate_series %r: expected a particles.RateSeries or None" % (rate_series,))
    if model not in ('field', 'rig'):
        raise ValueError("a rate series needs particle model 'field' or 'rig': the i.i.d. model has no time")
    R = rate_series.rate
    if R.ndim != 1 or len(R) < 2:
        raise ValueError("rate series: rate must hold n + 1 values with n >= 1, got shape %r" % (R.shape,))
    n = len(R) - 1
    if n > RATE_MAX_N:
        raise ValueError("rate series: n = %d is beyond 2^20 intervals" % n)
    if rate_series.frame0 < 0 or rate_series.frame0 + n > 2 ** 32:
        raise ValueError("rate series: frame0 %d + n %d must lie in 0 .. 2^32" % (rate_series.frame0, n))
    if not np.isfinite(R).all() or (R < 0).any():
        raise ValueError("rate series: every rate must be finite and >= 0 (mm/hr)")
    peak = rate_series.peak
    if not np.isfinite(peak) or not peak > 0 or peak < R.max():
        raise ValueError("rate series: peak %r must be finite, > 0 and >= max(rate) = %r" % (peak, float(R.max())))
    if frames is not None and not rate_series.covers(np.asarray(frames, np.int64) & 0xFFFFFFFF).all():
        raise ValueError("time index outside the rate series' frames %d .. %d" % (rate_series.frame0, rate_series.frame0 + n - 1))
    return rate_series


def shower_series(n, cam_hz, peak, low, period_s, frame0=0, phase=0.0):
    """A RateSeries of n intervals at cam_hz frames per second: a shower that swings between `low` and `peak` mm/hr once every
    `period_s` seconds, rate[i] = low + (peak - low) (1 - cos(2 pi (i / cam_hz) / period_s + phase)) / 2 (never above peak), with
    `peak` the series' peak.  A helper that makes data, like gust_series: the statements take any series."""
    n, cam_hz, peak, low, period_s, phase = int(n), float(cam_hz), float(peak), float(low), float(period_s), float(phase)
    if n < 1 or n > RATE_MAX_N:
        raise ValueError("shower_series: n must be 1 .. 2^20, got %d" % n)
    if not (np.isfinite(cam_hz) and cam_hz > 0 and np.isfinite(period_s) and period_s > 0 and np.isfinite(phase)):
        raise ValueError("shower_series: cam_hz > 0, period_s > 0 and phase must be finite")
    if not (np.isfinite(peak) and np.isfinite(low) and peak > 0 and 0 <= low <= peak):
        raise ValueError("shower_series: 0 <= low <= peak, peak > 0 (mm/hr)")
    i = np.arange(n + 1, dtype=np.float64)
    rate = low + (peak - low) * (1.0 - np.cos(2.0 * np.pi * (i / cam_hz) / period_s + phase)) / 2.0
    return _check_rate_series(RateSeries(frame0, np.minimum(np.maximum(rate, 0.0), peak), peak=peak))


def _rate_alive(rate_series, k, tau, cam_hz, D, w):
    """rr_particles.h rate_birth / rate_alive: whether the lives that began `tau` seconds before time index k, of drops of
    diameter D (mm) with the acceptance word w (word 3 of the life's block 1), are kept (module docstring): look up, interpolate,
    det_exp, compare -- one operation per step."""
    L = rate_series.dlam()
    m = (int(k) & 0xFFFFFFFF) - rate_series.frame0
    if not 0 <= m < rate_series.n:
        raise ValueError("time index %d is outside the rate series' frames %d .. %d" % (
            int(k), rate_series.frame0, rate_series.frame0 + rate_series.n - 1))
    back = tau * float(cam_hz)
    sb = np.maximum(float(m) - back, 0.0)
    i = np.floor(sb)
    ii = i.astype(np.int64)
    fr = sb - i
    l0, l1 = L[ii], L[ii + 1]
    Lb = l0 + fr * (l1 - l0)
    return unit32(w) < det_exp(-(Lb * D))


def _project(cam, X, Y, depth, wd):
    """rr_particles.h project: (sensor position (n, 2), image width) of one streak end at camera-frame (X, Y), `depth` away."""
    W, H = float(cam.W), float(cam.H)
    return np.stack([W / 2.0 + (cam.fpx * X) / depth, H / 2.0 + (cam.fpx * Y) / depth], axis=1), (wd * cam.fpx) / depth


def _records(n, wp1, wp2, wd, ip1, iw1, ip2, iw2):
    rec = np.zeros(n, PARTICLE_DTYPE)
    rec['pid'] = np.arange(n)
    rec['wp1'] = np.stack(wp1, axis=1)
    rec['wp2'] = np.stack(wp2, axis=1)
    rec['wd1'] = rec['wd2'] = wd
    rec['ip1'], rec['iw1'], rec['ip2'], rec['iw2'] = ip1, iw1, ip2, iw2
    return rec


def make_particles(cam, dgrid, cdf, n, frame, seed, wind_sigma=1.0, margin=0.05, min_px=1.0, z_far=15.0, wind=(0.0, 0.0)):
    """The n particles of simulated frame `frame` as PARTICLE_DTYPE records: the numpy statement of
    rr_particles.h make_particle (same operations, same order)."""
    if n == 0:
        return np.zeros(0, PARTICLE_DTYPE)
    i = np.arange(n, dtype=np.uint64)
    k0, k1 = _key(seed)
    a = philox4x32(i, frame, 0, 0, k0, k1)
    b = philox4x32(i, frame, 1, 0, k0, k1)
    c = philox4x32(i, frame, 2, 0, k0, k1)
    W, H = float(cam.W), float(cam.H)
    D = sample_diameter(dgrid, cdf, unit32(a[0]))                                # mm
    wd = D * 1e-3
    z_max = _slot_z_max(cam, wd, min_px, z_far)
    u1, u2, u3 = unit32(a[1]), unit32(a[2]), unit32(a[3])
    depth = np.maximum(z_max * np.maximum(np.maximum(u1, u2), u3), 0.05)        # uniform in the frustum volume
    lo_x, hi_x, lo_y, hi_y = -margin * W, (1.0 + margin) * W, -margin * H, (1.0 + margin) * H
    px = lo_x + (hi_x - lo_x) * unit32(b[0])
    py = lo_y + (hi_y - lo_y) * unit32(b[1])                                     # from the bottom
    X = ((px - W / 2.0) * depth) / cam.fpx
    Y = ((py - H / 2.0) * depth) / cam.fpx
    Z = -depth
    vx, vz = _drift(_block_wind(c, wind_sigma), cam.speed, wind)
    t = cam.exposure
    X2 = X + vx * t
    Y2 = Y - terminal_velocity(D) * t
    Z2 = Z + vz * t
    ip2, iw2 = _project(cam, X2, Y2, np.maximum(-Z2, 0.05), wd)
    return _records(n, [X, Y, Z], [X2, Y2, Z2], wd, np.stack([px, py], axis=1), (wd * cam.fpx) / depth, ip2, iw2)


def _settings_key(cam, rate):
    return (rate, cam.fpx, cam.W, cam.H)


def _per_settings(options, fallrate, n_frames, min_px, z_far, margin, make):
    """make(cam, rate, n) once per distinct settings (fall rate, camera) of the run, n = the distinct settings before it:
    (what it returned in first-use order, its index per simulated frame)."""
    keys, made, idx = {}, [], np.zeros(n_frames, np.int32)
    for k in range(n_frames):
        cam, rate = _frame_settings(options, fallrate, k, min_px, z_far, margin)
        tk = _settings_key(cam, rate)
        if tk not in keys:
            keys[tk] = len(made)
            made.append(make(cam, rate, len(made)))
        idx[k] = keys[tk]
    return made, idx


def _poisson(seed, salt, mean):
    return int(np.random.RandomState((int(seed) * 1000003 + salt) % (2 ** 32)).poisson(mean))


def field_slot_counts(options, fallrate, n_frames, seed=0, min_px=1.0, z_far=15.0, margin=0.05, count=None):
    """Particle slots of the field model per simulated frame: ONE Poisson draw per distinct settings (fall rate, camera)
    of the run around three times the expected count -- frames with the same settings share their slots -- or
    3 * `count` (`count`: the expected number of particles in the frustum, as for the i.i.d. model)."""
    if count is not None:
        return np.full(n_frames, 3 * int(count), np.int64)
    drawn, idx = _per_settings(options, fallrate, n_frames, min_px, z_far, margin, lambda cam, rate, n: _poisson(
        seed, 999983 + n, 3.0 * expected_count(cam, rate, min_px, z_far, margin)[0]))
    return np.asarray(drawn, np.int64)[idx]


def _slot_draw(cam, dgrid, cdf, j, key, min_px, z_far):
    """rr_particles.h slot_draw: what slot j is for good, from block (j, 0, 0, 1): (D in mm, phase, wd in m, z_max)."""
    a = philox4x32(j, 0, 0, 1, *key)
    D = sample_diameter(dgrid, cdf, unit32(a[0]))
    wd = D * 1e-3
    return D, unit32(a[1]), wd, _slot_z_max(cam, wd, min_px, z_far)


def _slot_fall(cam, cam_hz, k, j, key, D, wy, phase, wind_sigma):
    """rr_particles.h slot_fall: where slot j is in its fall through a box of height wy at time index k:
    (v, life g, age, tau, the life's block 1, the life's wind)."""
    v = terminal_velocity(D)
    T = wy / v
    t = float(int(k) & 0xFFFFFFFF) / float(cam_hz)
    s = t / T + phase
    g = np.floor(s)
    age = s - g
    tau = age * T
    b = philox4x32(*_life_counter(j, g, 1), *key)
    c = philox4x32(*_life_counter(j, g, 2), *key)
    return v, g, age, tau, b, _block_wind(c, wind_sigma)


def make_field_particles(cam, dgrid, cdf, n_slots, k, seed, cam_hz, wind_sigma=1.0, margin=0.05, min_px=1.0, z_far=15.0,
                         cull=True, wind=(0.0, 0.0), gusts=None, rate_series=None):
    """The field model's particles of time index `k` (t = k / cam_hz) under the settings `cam` / `cdf`: the numpy statement
    of rr_particles.h make_field_particle (same operations, same order).  Returns (PARTICLE_DTYPE records with pid = slot,
    life per record); with `cull` only the slots inside the frustum, in ascending slot order.  `rate_series`: `cdf` and
    n_slots are the peak's, and a life the series rejects is culled like a slot outside the frustum."""
    if n_slots == 0:
        return np.zeros(0, PARTICLE_DTYPE), np.zeros(0, np.float64)
    j = np.arange(n_slots, dtype=np.uint64)
    key = _key(seed)
    D, phase, wd, z_max = _slot_draw(cam, dgrid, cdf, j, key, min_px, z_far)
    W, H = float(cam.W), float(cam.H)
    hx, hy = ((0.5 + margin) * W) / cam.fpx, ((0.5 + margin) * H) / cam.fpx
    bx, by = hx * z_max, hy * z_max
    wx, wy = 2.0 * bx, 2.0 * by
    v, g, age, tau, b, wind_life = _slot_fall(cam, cam_hz, k, j, key, D, wy, phase, wind_sigma)
    vx, vz = _drift(wind_life, cam.speed, wind, gusts)
    ex, ez = vx, vz                                            # the velocity of the streak's end
    if gusts is None:
        qx = unit32(b[0]) + (vx * tau) / wx
        qz = unit32(b[1]) - (vz * tau) / z_max
    else:
        dG, ge = _gust_terms(_check_gusts(gusts, cam_hz), k, tau, cam_hz)
        qx = unit32(b[0]) + (vx * tau + dG[:, 0]) / wx
        qz = unit32(b[1]) - (vz * tau + dG[:, 1]) / z_max
        ex, ez = vx + ge[0], vz + ge[1]
    fx, fz = qx - np.floor(qx), qz - np.floor(qz)
    X = fx * wx - bx
    Y = by - age * wy
    zr = fz * z_max
    ax, ay = hx * zr, hy * zr
    inside = (-ax <= X) & (X <= ax) & (-ay <= Y) & (Y <= ay)
    if rate_series is not None:
        inside = inside & _rate_alive(_check_rate_series(rate_series), k, tau, cam_hz, D, b[3])
    depth = np.maximum(zr, 0.05)
    Z = -depth
    e = cam.exposure
    X2 = X + ex * e
    Y2 = Y - v * e
    Z2 = Z + ez * e
    rec = _records(n_slots, [X, Y, Z], [X2, Y2, Z2], wd, *_project(cam, X, Y, depth, wd), *_project(cam, X2, Y2, np.maximum(-Z2, 0.05), wd))
    if cull:
        return rec[inside], g[inside]
    return rec, g


def field_kinematics(cam, dgrid, cdf, slots, lives, seed, wind_sigma=1.0, margin=0.05, min_px=1.0, z_far=15.0, wind=(0.0, 0.0),
                     gusts=None):
    """Velocity (n, 3) in m/s (x right, y up, z towards the camera) of the given slots in the given lives, and the slots'
    boxes (n, 3): full width, full height, depth -- what tests compare a track's displacement with.  With `gusts` the velocity
    is the drop's own against the air, (vx, -v, vz) with both mean-wind additions formed: a frame's gust velocity ge and the
    air's step G[m + 1] - G[m] depend on the time index and are added by the caller."""
    j = np.asarray(slots, np.uint64)
    key = _key(seed)
    D, _, _, z_max = _slot_draw(cam, dgrid, cdf, j, key, min_px, z_far)
    hx, hy = ((0.5 + margin) * float(cam.W)) / cam.fpx, ((0.5 + margin) * float(cam.H)) / cam.fpx
    vx, vz = _drift(_block_wind(philox4x32(*_life_counter(j, lives, 2), *key), wind_sigma), cam.speed, wind, gusts)
    vel = np.stack([vx, -terminal_velocity(D), np.full(len(j), float(vz))], axis=1)
    return vel, np.stack([2.0 * (hx * z_max), 2.0 * (hy * z_max), z_max], axis=1)


def field_frame(options, fallrate, k, seed=0, min_px=1.0, z_far=15.0, margin=0.05, wind_sigma=1.0, count=None, n_sim=None,
                cull=True, wind=(0.0, 0.0), gusts=None, rate_series=None):
    """Frame `k` of a field-model run ALONE: (PARTICLE_DTYPE records with pid = slot id, life per record) of the particles
    inside the frustum -- the identity of a frame's particles.  Time index k, settings of simulated frame k % n_sim
    (n_sim: n_sim_frames(options) by default).  `generate(..., model='field')` is these frames one after the other.
    `rate_series`: `fallrate` is the series' peak."""
    n_sim = n_sim_frames(options) if n_sim is None else int(n_sim)
    ks = int(k) % n_sim
    cam, rate = _frame_settings(options, fallrate, ks, min_px, z_far, margin)
    _, dgrid, cdf, _ = expected_count(cam, rate, min_px, z_far, margin)
    n_slots = int(field_slot_counts(options, fallrate, ks + 1, seed, min_px, z_far, margin, count)[ks])
    if rate_series is None:
        return make_field_particles(cam, dgrid, cdf, n_slots, k, seed, cam.hz, wind_sigma, margin, min_px, z_far, cull, wind=wind, gusts=gusts)
    return make_field_particles(cam, dgrid, cdf, n_slots, k, seed, cam.hz, wind_sigma, margin, min_px, z_far, cull, wind=wind, gusts=gusts,
                                rate_series=rate_series)


# ---- the RIG model: one field, several cameras (module docstring) --------------------------------------------------
def rig_expected_count(cam, fallrate, box, min_px=1.0, z_far=15.0, n_grid=N_GRID):
    """(expected number of SLOTS, diameter grid, its sampling CDF, z_max per diameter) of the rig model: N(D) times the volume
    of the slot's box (2 r z_max)^2 (2 (r_y z_max + o_y)), `box` = (r, r_y, o_y)."""
    r, r_y, o_y = (float(v) for v in box)
    d = np.linspace(D_MIN, D_MAX, n_grid)
    z_max = np.minimum(d * 1e-3 * cam.fpx / min_px, z_far)
    w = 2.0 * (r * z_max)
    vol = (w * w) * (2.0 * (r_y * z_max + o_y))
    total, cdf = _diameter_cdf(N0 * det_exp(-mp_lambda(fallrate) * d) * vol, d)
    return total, d, cdf, z_max


def _rig_box(rig, cam, margin):
    return tuple(float(v) for v in rig.box(cam, margin))


def rig_run_box(options, fallrate, n_frames, rig, min_px=1.0, z_far=15.0, margin=0.05):
    """The ONE box (r, r_y, o_y) of a run (rr_set_particle_rig holds one): Rig.box of the run's camera.  A run whose simulated
    frames change the camera (cam_focal steps) has no single box and is refused."""
    boxes = {_rig_box(rig, _frame_settings(options, fallrate, k, min_px, z_far, margin)[0], margin) for k in range(n_frames)}
    if len(boxes) != 1:
        raise ValueError("the rig model needs one camera for the whole run: the focal length changes between simulated frames")
    return boxes.pop()


def rig_slot_counts(options, fallrate, n_frames, rig, seed=0, min_px=1.0, z_far=15.0, margin=0.05, count=None):
    """Particle slots of the rig model per simulated frame: ONE Poisson draw per distinct settings of the run around the
    expected number of slots (rig_expected_count) -- or, with `count` (the expected number of particles in ONE view's frustum,
    as for the other models), count x expected slots / expected particles, rounded."""
    def draw(cam, rate, n):
        mean = rig_expected_count(cam, rate, _rig_box(rig, cam, margin), min_px, z_far)[0]
        if count is not None:
            return int(round(int(count) * mean / expected_count(cam, rate, min_px, z_far, margin)[0]))
        return _poisson(seed, 999979 + n, mean)
    drawn, idx = _per_settings(options, fallrate, n_frames, min_px, z_far, margin, draw)
    return np.asarray(drawn, np.int64)[idx]


def _tables(options, fallrate, n_frames, min_px, z_far, margin, table):
    """(d_grid, cdf [n_tables, N_GRID], table index per frame): table(cam, rate) = (_, d_grid, cdf, _) per distinct settings."""
    tabs, idx = _per_settings(options, fallrate, n_frames, min_px, z_far, margin, lambda cam, rate, n: table(cam, rate))
    return (tabs[-1][1] if tabs else None), np.ascontiguousarray(np.stack([t[2] for t in tabs])), idx


def rig_tables(options, fallrate, n_frames, rig, min_px=1.0, z_far=15.0, margin=0.05):
    """diameter_tables for the rig model: (d_grid, cdf [n_tables, N_GRID], table index per frame)."""
    return _tables(options, fallrate, n_frames, min_px, z_far, margin,
                   lambda cam, rate: rig_expected_count(cam, rate, _rig_box(rig, cam, margin), min_px, z_far))


def rig_state(cam, dgrid, cdf, n_slots, k, seed, cam_hz, box, wind_sigma=1.0, min_px=1.0, z_far=15.0, wind=(0.0, 0.0), gusts=None,
              rate_series=None):
    """The rig-frame state of every slot at time index k -- the part of make_rig_particles no view enters (rr_particles.h
    make_rig_slot): dict(D, z_max, b (half side in x and z), by, pos (n, 3), vel (n, 3) in m/s, life).  With `rate_series` also
    `alive`: whether the series keeps the slot's life -- one decision per slot, for every view."""
    r, r_y, o_y = (float(v) for v in box)
    j = np.arange(n_slots, dtype=np.uint64)
    key = _key(seed)
    D, phase, wd, z_max = _slot_draw(cam, dgrid, cdf, j, key, min_px, z_far)
    b = r * z_max
    by = r_y * z_max + o_y
    w, wy = 2.0 * b, 2.0 * by
    v, g, age, tau, bb, wind_life = _slot_fall(cam, cam_hz, k, j, key, D, wy, phase, wind_sigma)
    vx, vz = _drift(wind_life, cam.speed, wind, gusts)
    if gusts is None:
        qx = unit32(bb[0]) + (vx * tau) / w
        qz = unit32(bb[1]) + (vz * tau) / w
    else:                                                      # the slot's velocity carries the frame's gust: once per slot, for every view
        dG, ge = _gust_terms(_check_gusts(gusts, cam_hz, 'rig'), k, tau, cam_hz)
        qx = unit32(bb[0]) + (vx * tau + dG[:, 0]) / w
        qz = unit32(bb[1]) + (vz * tau + dG[:, 1]) / w
        vx, vz = vx + ge[0], float(vz) + ge[1]
    fx, fz = qx - np.floor(qx), qz - np.floor(qz)
    X = fx * w - b
    Y = by - age * wy
    Z = fz * w - b
    st = dict(D=D, wd=wd, z_max=z_max, b=b, by=by, life=g, pos=np.stack([X, Y, Z], axis=1),
              vel=np.stack([vx, -v, np.full(n_slots, float(vz))], axis=1))
    if rate_series is not None:
        st['alive'] = _rate_alive(_check_rate_series(rate_series, 'rig'), k, tau, cam_hz, D, bb[3])
    return st


def make_rig_particles(cam, dgrid, cdf, n_slots, k, seed, cam_hz, view, box, wind_sigma=1.0, margin=0.05, min_px=1.0, z_far=15.0,
                       cull=True, image=(0, 0), view_end=None, wind=(0.0, 0.0), gusts=None, rate_series=None):
    """The rig model's particles of time index `k` as view `view` = (R [9] row-major rig -> camera, c [3]) sees them: the numpy
    statement of rr_particles.h make_rig_slot + rig_view_particle (traj_view_start, rig_view_end; same operations, same order).  `box` = (r, r_y, o_y).
    Returns (PARTICLE_DTYPE records in the CAMERA's frame with pid = slot, life per record); with `cull` only the slots the
    view keeps, in ascending slot order.  `image` = (ix, iz) looks at the lattice image ix, iz periods away from the nearest
    one instead (tests: with the host's r no such image is ever inside the frustum).

    `view_end` = (R1, c1): the view's pose at the END of the exposure (a trajectory, module docstring; rr_particles.h
    traj_view_start + traj_view_end): the streak's end is R1 ((d + velocity x exposure) - (c1 - c)), d the start's wrapped
    offset.  With view_end equal to `view` the subtraction is - 0.0: the bits of view_end=None."""
    if n_slots == 0:
        return np.zeros(0, PARTICLE_DTYPE), np.zeros(0, np.float64)
    R = [float(v) for v in np.asarray(view[0], np.float64).reshape(9)]
    c = [float(v) for v in np.asarray(view[1], np.float64).reshape(3)]
    if rate_series is None:
        st = rig_state(cam, dgrid, cdf, n_slots, k, seed, cam_hz, box, wind_sigma, min_px, z_far, wind=wind, gusts=gusts)
    else:
        st = rig_state(cam, dgrid, cdf, n_slots, k, seed, cam_hz, box, wind_sigma, min_px, z_far, wind=wind, gusts=gusts, rate_series=rate_series)
    W, H = float(cam.W), float(cam.H)
    hx, hy = ((0.5 + margin) * W) / cam.fpx, ((0.5 + margin) * H) / cam.fpx
    b, z_max, wd = st['b'], st['z_max'], st['wd']
    w = 2.0 * b
    dx = st['pos'][:, 0] - c[0]
    dy = st['pos'][:, 1] - c[1]
    dz = st['pos'][:, 2] - c[2]
    dx = dx - np.floor((dx + b) / w) * w                       # the lattice image nearest to the camera
    dz = dz - np.floor((dz + b) / w) * w
    if image[0] or image[1]:
        dx = dx + float(image[0]) * w
        dz = dz + float(image[1]) * w
    xc = (R[0] * dx + R[1] * dy) + R[2] * dz
    yc = (R[3] * dx + R[4] * dy) + R[5] * dz
    zc = (R[6] * dx + R[7] * dy) + R[8] * dz
    zr = -zc                                                    # depth along the view's axis
    ax, ay = hx * zr, hy * zr
    inside = (zr > 0.0) & (zr <= z_max) & (-ax <= xc) & (xc <= ax) & (-ay <= yc) & (yc <= ay)
    if rate_series is not None:                                 # a rejected slot is kept by no view
        inside = inside & st['alive']
    depth = np.maximum(zr, 0.05)
    e = cam.exposure
    ex = dx + st['vel'][:, 0] * e
    ey = dy + st['vel'][:, 1] * e
    ez = dz + st['vel'][:, 2] * e
    if view_end is not None:                                    # the camera's own displacement; the same lattice image, not re-wrapped
        c1 = [float(v) for v in np.asarray(view_end[1], np.float64).reshape(3)]
        ex = ex - (c1[0] - c[0])
        ey = ey - (c1[1] - c[1])
        ez = ez - (c1[2] - c[2])
        R = [float(v) for v in np.asarray(view_end[0], np.float64).reshape(9)]
    X2 = (R[0] * ex + R[1] * ey) + R[2] * ez
    Y2 = (R[3] * ex + R[4] * ey) + R[5] * ez
    Z2 = (R[6] * ex + R[7] * ey) + R[8] * ez
    rec = _records(n_slots, [xc, yc, -depth], [X2, Y2, Z2], wd, *_project(cam, xc, yc, depth, wd),
                   *_project(cam, X2, Y2, np.maximum(-Z2, 0.05), wd))
    if cull:
        return rec[inside], st['life'][inside]
    return rec, st['life']


def _traj_cam(cam):
    """The camera of a frame under a trajectory: speed 0 -- the trajectory says how the camera moves."""
    out = FrameCamera.__new__(FrameCamera)
    out.__dict__.update(cam.__dict__)
    out.speed = 0.0
    return out


def rig_frame(options, fallrate, k, rig, view, seed=0, min_px=1.0, z_far=15.0, margin=0.05, wind_sigma=1.0, count=None, n_sim=None,
              cull=True, image=(0, 0), trajectory=None, box=None, wind=(0.0, 0.0), gusts=None, rate_series=None):
    """Frame (k, view) of a rig-model run ALONE: (records with pid = slot, life per record), like field_frame.  With
    `trajectory` (trajectory.Trajectory): the view's composed poses of time index k, the trajectory's box and slot counts, speed 0.
    `box`: another box than the run's (tests)."""
    n_sim = n_sim_frames(options) if n_sim is None else int(n_sim)
    ks = int(k) % n_sim
    cam, rate = _frame_settings(options, fallrate, ks, min_px, z_far, margin)
    src = rig if trajectory is None else trajectory.bind(rig)
    run_box = _rig_box(src, cam, margin)
    _, dgrid, cdf, _ = rig_expected_count(cam, rate, run_box, min_px, z_far)
    n_slots = int(rig_slot_counts(options, fallrate, ks + 1, src, seed, min_px, z_far, margin, count)[ks])
    box = run_box if box is None else tuple(float(v) for v in box)
    pose, view_end = rig.views[int(view)], None
    if trajectory is not None:
        po = trajectory.compose(rig, cam.exposure)[int(k), int(view)]
        cam, pose, view_end = _traj_cam(cam), (po['R0'], po['c0']), (po['R1'], po['c1'])
    return make_rig_particles(cam, dgrid, cdf, n_slots, k, seed, cam.hz, pose, box, wind_sigma, margin, min_px, z_far, cull, image,
                              view_end=view_end, wind=wind, gusts=gusts, rate_series=rate_series)


def rig_run_sims(sims, k_idx, n_active):
    """The records of instants `k_idx` of a rig-model run, n_active consecutive records per instant (frame i = active view
    i % n_active of instant i / n_active): field_run_sims with every instant repeated."""
    return field_run_sims(sims, np.repeat(np.asarray(k_idx, np.int64), int(n_active)))


def generate(options, fallrate, n_frames, seed=0, min_px=1.0, z_far=15.0, margin=0.05, wind_sigma=1.0, count=None, model='iid',
             wind=(0.0, 0.0), gusts=None, rate_series=None):
    """(frames, drops) record arrays of `n_frames` camera frames.  `count`: force that many drops per frame instead
    of the Poisson-distributed physical count.  model='field': the persistent field (module docstring), frame k at time
    k / cam_hz under the settings of simulated frame k; pid is then the slot id.  (The rig model has no particle file: its
    frames are made per view, rig_frame.)"""
    frames = np.zeros(n_frames, PARTICLE_FRAME_DTYPE)
    _check_model(model)
    if gusts is not None and model == 'iid':
        raise ValueError("a gust series needs particle model 'field' or 'rig': the i.i.d. model has no time")
    if rate_series is not None:                                # (`fallrate` is the series' peak: the slots and tables are the peak's)
        _check_rate_series(rate_series, model, frames=range(n_frames) if model == 'field' else None)
    if model == 'rig':
        raise ValueError("particle model 'rig' writes no particle file: use rig_frame / expected_records (one table per view)")
    if model == 'field':
        counts = field_slot_counts(options, fallrate, n_frames, seed, min_px, z_far, margin, count)
    else:
        counts = frame_counts(options, fallrate, n_frames, seed, min_px, z_far, margin, count)
    chunks = []
    first = 0
    tables = {}
    for k in range(n_frames):
        cam, rate = _frame_settings(options, fallrate, k, min_px, z_far, margin)
        tk = _settings_key(cam, rate)
        if tk not in tables:
            tables[tk] = expected_count(cam, rate, min_px, z_far, margin)
        _, dgrid, cdf, _ = tables[tk]
        n = int(counts[k])
        if model == 'field':
            rec, _ = make_field_particles(cam, dgrid, cdf, n, k, seed, cam.hz, wind_sigma, margin, min_px, z_far, wind=wind, gusts=gusts,
                                          rate_series=rate_series)
            n = len(rec)
        else:
            rec = make_particles(cam, dgrid, cdf, n, k, seed, wind_sigma, margin, min_px, z_far, wind=wind)
        frames[k] = (k, int(round(cam.exposure * 1e6)), int(round(k * 1e6 / cam.hz)), n, first, n)
        chunks.append(rec)
        first += n
    return frames, (np.concatenate(chunks) if chunks else np.zeros(0, PARTICLE_DTYPE))


# ---- the same run described to the library (rr_set_particle_tables / rr_sim_frame) -----------------------------------
def diameter_tables(options, fallrate, n_frames, min_px=1.0, z_far=15.0, margin=0.05):
    """(d_grid [N_GRID], cdf [n_tables, N_GRID], table index per frame): one table per distinct (fall rate, camera)."""
    return _tables(options, fallrate, n_frames, min_px, z_far, margin, lambda cam, rate: expected_count(cam, rate, min_px, z_far, margin))


def sim_frames(options, fallrate, n_frames, render_scale=1, seed=0, draw_seeds=None, min_px=1.0, z_far=15.0, margin=0.05,
               wind_sigma=1.0, count=None, frame_ids=None, model='iid', rig=None, trajectory=None):
    """SIM_FRAME_DTYPE records (hip_backend: the numpy mirror of rr_sim_frame) of `n_frames` camera frames + the tables
    they refer to: (sims, d_grid, cdf).  draw_seeds: np.random.seed(...) of the renderer's per-drop draws per frame
    (generator.py:318: the frame's index; default: the frame number).  model='field' (rr_set_particle_model): n_particles
    is the run's slot count under the frame's settings and `frame` the TIME index; a rendered frame f of a run takes the
    record of simulated frame f % n_sim with frame = f (field_run_sims).  model='rig' with `rig` (rig.Rig): likewise with the
    rig's own tables and slot counts (rig_tables, rig_slot_counts); an instant's views share its record up to draw_seed
    (rig_run_sims).  With `trajectory` (trajectory.Trajectory; rig model only): the slot counts and tables take
    Trajectory.box, and speed_mps is 0 -- the trajectory says how the camera moves."""
    from .. import hip_backend
    _check_model(model)
    if trajectory is not None and model != 'rig':
        raise ValueError("a trajectory needs particle model 'rig' (a single camera: Rig.from_spec('mono'))")
    if model == 'rig':
        if rig is None:
            raise ValueError("particle model 'rig' needs rig= (rig.Rig)")
        if trajectory is not None:
            rig = trajectory.bind(rig)
        rig_run_box(options, fallrate, n_frames, rig, min_px, z_far, margin)
        dgrid, cdf, tab = rig_tables(options, fallrate, n_frames, rig, min_px, z_far, margin)
        counts = rig_slot_counts(options, fallrate, n_frames, rig, seed, min_px, z_far, margin, count)
    else:
        dgrid, cdf, tab = diameter_tables(options, fallrate, n_frames, min_px, z_far, margin)
        counts = (field_slot_counts if model == 'field' else frame_counts)(options, fallrate, n_frames, seed, min_px, z_far, margin, count)
    sims = np.zeros(n_frames, hip_backend.SIM_FRAME_DTYPE)
    k0, k1 = _key(seed)
    for k in range(n_frames):
        cam, _ = _frame_settings(options, fallrate, k, min_px, z_far, margin)
        s = sims[k]
        s['sensor_w'], s['sensor_h'], s['render_scale'], s['n_particles'] = cam.W, cam.H, render_scale, counts[k]
        s['key0'], s['key1'], s['frame'] = k0, k1, k if frame_ids is None else frame_ids[k]
        s['draw_seed'] = k if draw_seeds is None else draw_seeds[k]
        s['table'] = tab[k]
        s['fpx'], s['exposure_s'], s['speed_mps'] = cam.fpx, cam.exposure, 0.0 if trajectory is not None else cam.speed
        s['wind_sigma'], s['margin'], s['min_px'], s['z_far'] = wind_sigma, margin, min_px, z_far
    return sims, dgrid, cdf


def field_run_sims(sims, f_idx):
    """The records of rendered frames `f_idx` of a field-model run: the settings of simulated frame f % len(sims), the time
    index and the draw seed f."""
    f = np.asarray(f_idx, np.int64)
    out = np.ascontiguousarray(sims[f % len(sims)])
    out['frame'] = f.astype(np.uint32)
    out['draw_seed'] = f.astype(np.uint32)
    return out


def _loaded_table(s, dgrid, cdf, db, dataset, model='iid', cam_hz=None, rig=None, view=0, draws='stream', jitter=0.0, trajectory=None,
                  wind=(0.0, 0.0), gusts=None, rate_series=None):
    """(streak table, W, H) of one rr_sim_frame record the host's way: make_particles -> DBManager.load_streaks_from_records
    (the loader's derived fields) on the rendered frame.  draws='counter': the table also carries `pick`, the counter-based
    texture pick of every row (counter_picks of the row's particle); with `jitter`, `jitter_g`: the row's counter_jitter."""
    from ..common import bad_weather as bw
    cam = type('Cam', (), dict(W=int(s['sensor_w']), H=int(s['sensor_h']), fpx=float(s['fpx']), exposure=float(s['exposure_s']),
                               speed=float(s['speed_mps'])))()
    seed = int(s['key0']) | (int(s['key1']) << 32)
    life = None
    k, margin = int(s['frame']), float(s['margin'])
    tab, n = cdf[int(s['table'])], int(s['n_particles'])
    kw = dict(wind_sigma=float(s['wind_sigma']), margin=margin, min_px=float(s['min_px']), z_far=float(s['z_far']), wind=wind)
    if model == 'rig':
        pose, box, view_end = rig.views[int(view)] if trajectory is None else None, rig, None
        if trajectory is not None:
            po = trajectory.compose(rig, cam.exposure)
            if k >= len(po):
                raise ValueError("time index %d is outside the trajectory's %d poses" % (k, len(po)))
            po = po[k, int(view)]
            pose, box, view_end = (po['R0'], po['c0']), trajectory.bind(rig), (po['R1'], po['c1'])
        rec, life = make_rig_particles(cam, dgrid, tab, n, k, seed, float(cam_hz), pose, _rig_box(box, cam, margin), view_end=view_end, gusts=gusts,
                                       rate_series=rate_series, **kw)
    elif model == 'field':
        rec, life = make_field_particles(cam, dgrid, tab, n, k, seed, float(cam_hz), gusts=gusts, rate_series=rate_series, **kw)
    else:
        rec = make_particles(cam, dgrid, tab, n, k, seed, **kw)
    fr = np.zeros(1, PARTICLE_FRAME_DTYPE)
    fr[0] = (0, 0, 0, len(rec), 0, len(rec))
    m = bw.DBManager()
    m.ratio = db.ratio
    rs = int(s['render_scale'])
    W, H = int(s['sensor_w']) // rs, int(s['sensor_h']) // rs
    m.load_streaks_from_records(fr, rec, dataset, {"render_scale": rs}, [W, H])
    table = m.streaks_simulator[0].table
    if draws == 'counter':
        picks = counter_picks(seed, rec['pid'], int(s['frame']), life)
        table.pick = picks[np.searchsorted(rec['pid'], table.pid)]      # (pid ascends: particle index, or slot)
    if jitter:
        gs = counter_jitter(seed, rec['pid'], int(s['frame']), life)
        table.jitter_g = gs[np.searchsorted(rec['pid'], table.pid)]
    return table, m, W, H


def expected_records(sims, dgrid, cdf, db, dataset='kitti', noise_std=0.0, noise_scale=0.0, run=None, model='iid', cam_hz=None,
                     rig=None, view=None, draws='stream', jitter=0.0, trajectory=None, wind=(0.0, 0.0),
                     gusts=None, rate_series=None):
    """What rr_generate_drops_device must leave in HBM for these frames: per frame the rr_drop records (DROP_DTYPE) made the
    host's way -- make_particles -> DBManager.load_streaks_from_records (the loader's derived fields) ->
    hip_backend.pack_frame (frame filter + the frame's random draws) with the exact rotation terms.  `db`: a DBManager
    with the streak database loaded (texture ratios).

    Angular noise (noise_std and noise_scale both non-zero, rr_set_particle_noise): `run` = (run_frame, run_seed), the
    run's entries in order.  A frame with run_pos p >= 1 is entry p - 1: its simulated frame's pristine streaks are
    stepped (noise_step) through every earlier entry of the same simulated frame, in run order, then through its own
    entry, whose records it gets -- the reference's in-place rotation of the shared table (generator.py:152-161)
    replayed from scratch, so the result depends on nothing but the frame.

    model='field' with the run's `cam_hz` (rr_set_particle_model): the records of the field model's frames
    (make_field_particles: slots inside the frustum in ascending order, then the same loader, filter and draws).

    model='rig' with `rig` (rig.Rig) and `cam_hz` (rr_set_particle_rig): record i is the frame of view `view[i % len(view)]`
    -- `view`: the active list as the library gets it (default: every view of the rig in order), or one view's number for
    records that are all of that view.

    draws='counter' (rr_set_particle_draws RR_DRAWS_COUNTER): the same records with tex_index = 10 * texture_bucket(ratio) +
    counter_picks of the drop instead of the stream's randint; draw_seed is ignored; no angular noise, no run_pos.

    trajectory= (trajectory.Trajectory; model='rig', rr_set_particle_trajectory): record i is view view[i % len(view)] under the
    composed poses of time index sims[i]['frame'] (make_rig_particles view_end=), in the trajectory's box.

    jitter=DEG (rr_set_particle_jitter; every model, both draws): the records above, then every kept non-Big one turned by
    DEG * counter_jitter of its drop (jitter_records).  jitter=0: the records above.  Not with noise_std / noise_scale / run, and
    run_pos must be 0.

    wind=(wx, wz) (rr_set_particle_wind; every model, both draws, with jitter, rig and trajectory): the records of the particles
    made under that mean wind (module docstring).  (0, 0): the records above.

    gusts=GustSeries (rr_set_particle_gusts; field and rig models, both draws, with jitter, wind and trajectory): the records of the
    particles made under that gust series; every record's frame must lie inside it and run_pos must be 0.  None: the records above.

    rate_series=RateSeries (rr_set_particle_rate_series; field and rig models, both draws, with jitter, wind, gusts and trajectory):
    the records of the lives that series keeps -- `sims` and `cdf` are the peak rate's; every record's frame must lie inside the
    series and run_pos must be 0.  None: the records above."""
    from .. import hip_backend
    _check_model(model)
    wind = _check_wind(wind)
    if gusts is not None:
        _check_gusts(gusts, cam_hz, model, frames=[int(s['frame']) for s in sims])
        if any(int(s['run_pos']) != 0 for s in sims):
            raise ValueError("a gust series: run_pos must be 0")
    if rate_series is not None:
        _check_rate_series(rate_series, model, frames=[int(s['frame']) for s in sims])
        if any(int(s['run_pos']) != 0 for s in sims):
            raise ValueError("a rate series: run_pos must be 0")
    noisy = bool(noise_std) and bool(noise_scale)
    jitter = _check_jitter(jitter, noisy, run)
    _check_draws(draws, noisy)
    if trajectory is not None and model != 'rig':
        raise ValueError("a trajectory needs particle model 'rig'")
    if model in ('field', 'rig') and (noisy or cam_hz is None):
        raise ValueError("the %s model needs cam_hz and has no angular noise" % model)
    views = [0]
    if model == 'rig':
        if rig is None:
            raise ValueError("particle model 'rig' needs rig= (rig.Rig)")
        views = list(range(len(rig.views))) if view is None else [int(v) for v in np.atleast_1d(view)]
        if len(sims) % len(views):
            raise ValueError("%d records are not a multiple of the %d active views" % (len(sims), len(views)))
    out = []
    for i, s in enumerate(sims):
        table, m, W, H = _loaded_table(s, dgrid, cdf, db, dataset, model, cam_hz, rig, views[i % len(views)], draws, jitter, trajectory, wind, gusts,
                                       rate_series)
        p = int(s['run_pos'])
        if jitter or draws == 'counter':
            if p != 0:
                raise ValueError("%s: run_pos must be 0 (frame %d)" % ("streak jitter" if jitter else "counter draws", i))
            rec = hip_backend.pack_frame(table, m, W, H, int(s['draw_seed']), rotation='exact')
            keep = hip_backend.filter_streaks(table, W, H)
            assert len(keep) == len(rec)
            if draws == 'counter':                            # (the stream's pick is overwritten: draw_seed is ignored)
                rec['tex_index'] = 10 * m.texture_bucket(table.ratio[keep]) + table.pick[keep]
            out.append(jitter_records(rec, table.jitter_g[keep], jitter) if jitter else rec)
            continue
        if not noisy or p == 0:
            out.append(hip_backend.pack_frame(table, m, W, H, int(s['draw_seed']), rotation='exact'))
            continue
        run_frame, run_seed = (np.asarray(v).astype(np.int64) for v in run)
        assert 1 <= p <= len(run_frame) and run_frame[p - 1] == int(s['frame']) and run_seed[p - 1] == int(s['draw_seed']), \
            'run_pos %d does not name this frame' % p
        ratio_db = np.asarray(db.ratio, np.float64)
        for j in range(p - 1):
            if run_frame[j] == run_frame[p - 1]:
                noise_step(table, W, H, ratio_db, int(run_seed[j]), noise_std, noise_scale)
        out.append(noise_step(table, W, H, ratio_db, int(s['draw_seed']), noise_std, noise_scale))
    return out


def run_table(sims, n_sim, f_name_idx):
    """(run_frame, run_seed) of a run whose entries are the frames f_name_idx in order (generator.py:304-321: simulated
    frame f % n_sim, draws seeded with f): rr_set_particle_noise's table."""
    f = np.asarray(f_name_idx, np.int64)
    return np.asarray(sims['frame'], np.uint32)[f % n_sim], f.astype(np.uint32)


def write_xml(path, frames, drops):
    """The file the reference's DBManager.load_streaks_from_xml reads (bad_weather.py:192-211).  Written under a temporary
    name and moved into place: a reader never sees half a file."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    fmt = ('    <streak pid="%d" wp1="(%.17g;%.17g;%.17g)" wp2="(%.17g;%.17g;%.17g)" wd1="%.17g" wd2="%.17g" '
           'ip1="(%.17g;%.17g)" ip2="(%.17g;%.17g)" iw1="%.17g" iw2="%.17g"/>')
    tmp = '%s.tmp%d' % (path, os.getpid())
    with open(tmp, 'w') as fh:
        fh.write('<?xml version="1.0" ?>\n<simulation>\n')
        for fr in frames:
            a, n = int(fr['first_drop']), int(fr['n_drops'])
            fh.write('  <frame id="%d" t="%d" d="%d" rs="%d">\n' % (fr['id'], fr['t'], fr['d'], fr['rs']))
            d = drops[a:a + n]
            if n:
                cols = np.column_stack([d['pid'].astype(np.float64), d['wp1'], d['wp2'], d['wd1'], d['wd2'], d['ip1'], d['ip2'],
                                        d['iw1'], d['iw2']])
                fh.write('\n'.join(fmt % ((int(r[0]),) + tuple(r[1:])) for r in cols.tolist()))
                fh.write('\n')
            fh.write('  </frame>\n')
        fh.write('</simulation>\n')
    os.replace(tmp, path)
    return path


def n_sim_frames(options):
    steps = options.get("sim_steps", {}) or {}
    n_steps = max([len(v) for v in steps.values()] + [0])
    return n_steps if options.get("sim_mode") == "steps" and n_steps else int(options["sim_duration"] * options["cam_hz"])


def simulate(sim, weather, n_frames=None, seed=0, force_recompute=False, model='iid'):
    """The role of the reference's tools/particles_simulation.process for ONE sequence: `sim` = common.db.sim(...)
    ({"path", "options"}), `weather` = {"weather": "rain", "fallrate": R}.  Writes
    <sim path>/<weather>/<R>mm/sim_camera0.xml unless it exists; returns its path."""
    options = sim["options"]
    out_dir = os.path.join(sim["path"], weather["weather"], '{}mm'.format(weather["fallrate"]))
    path = os.path.join(out_dir, 'sim_camera0.xml')
    if os.path.exists(path) and not force_recompute:
        return path
    if n_frames is None:
        n_frames = n_sim_frames(options)
    frames, drops = generate(options, weather["fallrate"], n_frames, seed=seed, model=model)
    return write_xml(path, frames, drops)
