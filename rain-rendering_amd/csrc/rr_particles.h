// rr_particles.h -- the rain-particle generator and the drop-table packer, per particle (SURVEY 8f "next" #4;
// BASELINE.json configs[4]: "in-kernel particle simulation (no XML)").
//
// `__host__ __device__` like rr_device.h: k_particles (rainhip.hip) runs these functions on gfx950, tests/hostemu
// compiles them with g++, and rain-rendering_amd/tools/particles.py states the same arithmetic in numpy (its bit-exact
// host statement; the model itself is documented there).  IEEE double, the evaluation order spelled out, no FMA
// contraction, + - * / sqrt rint floor only (sqrt is correctly rounded on gfx950 and in numpy); the one transcendental -- exp
// in the terminal velocity -- is rr::det_exp.
//
//   reference side: tools/simulation.py drives a closed-source simulator with the settings of common/db.py:41-70;
//   its XML (bad_weather.py:192-211) passes through the loader's derived fields (bad_weather.py:208-241) and the frame
//   filter of Generator.run (generator.py:413-420).  The last two are followed to the letter below.
#pragma once
#include "rr_device.h"

namespace rrsim {

using rr::det_exp;

// ---- Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> four 32-bit words ----
RR_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += W0;
    k1 += W1;
  }
}
// a 32-bit word as a number strictly inside (0, 1): (w + 1/2) / 2^32, exact in double
RR_HD double unit32(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

struct Particle {                 // what one <streak .../> element of the simulator's XML carries (bad_weather.py:192-211)
  double wp1[3], wp2[3];          // world position at the start / end of the exposure, camera at the origin looking along -z
  double wd;                      // diameter, metres
  double ip1[2], ip2[2];          // sensor position, pixels, origin bottom-left
  double iw1, iw2;                // image width, pixels
};

// terminal velocity of a drop of diameter d_mm, m/s (Atlas, Srivastava & Sekhon 1973)
RR_HD double terminal_velocity(double d_mm) { return 9.65 - 10.3 * det_exp(-0.6 * d_mm); }

// inverse-CDF sample of the diameter table: largest j with cdf[j] <= u (j <= n - 2), linear inside the cell
RR_HD double sample_diameter(const double* dgrid, const double* cdf, int n, double u) {
  int lo = 0, hi = n - 1;                       // invariant: cdf[lo] <= u (cdf[0] = 0 < u), answer in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid; else hi = mid;
  }
  const double slope = (dgrid[lo + 1] - dgrid[lo]) / (cdf[lo + 1] - cdf[lo]);
  return dgrid[lo] + (u - cdf[lo]) * slope;
}

// The counter-based texture pick (rr_set_particle_draws RR_DRAWS_COUNTER, tools/particles.py counter_picks): word 2 of the
// drop's Philox block 1 -- which no other draw reads -- scaled to 0 .. 9; tex_index = 10 * texture_bucket(ratio) + pick.
RR_HD int texture_pick(uint32_t w) { return (int)(((uint64_t)w * 10u) >> 32); }

// z_max(D): only drops that can show at least min_px wide are simulated (wd: the diameter in metres)
RR_HD double slot_z_max(const rr_sim_frame& sf, double wd) { return rr::dmin((wd * sf.fpx) / sf.min_px, sf.z_far); }

// horizontal wind from one Philox block: a centred sum of four uniforms scaled to unit variance (bell-shaped, bounded), times wind_sigma
RR_HD double block_wind(const uint32_t c[4], double wind_sigma) {
  const double s4 = ((unit32(c[0]) + unit32(c[1])) + (unit32(c[2]) + unit32(c[3]))) - 2.0;
  return (s4 * 1.7320508075688772) * wind_sigma;
}

// the pinhole projection of one streak end at camera-frame (X, Y), `depth` in front of the camera: sensor position (origin
// bottom-left) and image width of a drop of diameter wd
RR_HD void project(const rr_sim_frame& sf, double X, double Y, double depth, double wd, double ip[2], double& iw) {
  const double W = (double)sf.sensor_w, H = (double)sf.sensor_h;
  ip[0] = W / 2.0 + (sf.fpx * X) / depth;
  ip[1] = H / 2.0 + (sf.fpx * Y) / depth;
  iw = (wd * sf.fpx) / depth;
}

// ---- the MEAN WIND (rr_set_particle_wind, tools/particles.py wind=): the air's mean horizontal velocity (wx, wz), m/s ----
// In the axes of the particle world: x right, z toward the viewer -- the camera frame of the i.i.d. and field models, the rig
// frame of the rig model, the lattice's world frame under a trajectory.  WIND is a compile-time switch of every generator
// below, the way TRAJ is one of k_rig_particles: with WIND the drop's horizontal velocity is vx = wind_life + wx and
// vz = speed_mps + wz, each evaluated once, and those two take the place of the life's wind and of speed_mps wherever they
// enter.  WIND = false is the function as it was: wx and wz are not read (x + 0.0 is not x for x = -0.0, which block_wind
// gives at wind_sigma = 0, so the sums are not formed at all).  Slot counts, boxes, lives and tables do not depend on it.

// particle i of frame sf: three Philox blocks, counter = (i, frame, block, 0); *pick_word = the pick's word (b[2])
template <bool WIND = false>
RR_HD void make_particle(const rr_sim_frame& sf, const double* dgrid, const double* cdf, int n_grid, uint32_t i, Particle& p,
                         uint32_t* pick_word = nullptr, double wx = 0.0, double wz = 0.0) {
  uint32_t a[4] = {i, sf.frame, 0u, 0u}, b[4] = {i, sf.frame, 1u, 0u}, c[4] = {i, sf.frame, 2u, 0u};
  philox4x32_10(a, sf.key0, sf.key1);
  philox4x32_10(b, sf.key0, sf.key1);
  philox4x32_10(c, sf.key0, sf.key1);
  const double W = (double)sf.sensor_w, H = (double)sf.sensor_h;
  const double D = sample_diameter(dgrid, cdf, n_grid, unit32(a[0]));   // diameter (mm) from the table
  const double wd = D * 1e-3;
  const double z_max = slot_z_max(sf, wd);
  // uniform in the frustum's volume: the depth's density is 3 z^2 / z_max^3, the law of the largest of three uniforms
  const double u1 = unit32(a[1]), u2 = unit32(a[2]), u3 = unit32(a[3]);
  const double depth = rr::dmax(z_max * rr::dmax(rr::dmax(u1, u2), u3), 0.05);
  // position on the (slightly enlarged) sensor, from the bottom-left corner
  const double lo_x = -sf.margin * W, hi_x = (1.0 + sf.margin) * W, lo_y = -sf.margin * H, hi_y = (1.0 + sf.margin) * H;
  const double px = lo_x + (hi_x - lo_x) * unit32(b[0]);
  const double py = lo_y + (hi_y - lo_y) * unit32(b[1]);
  const double X = ((px - W / 2.0) * depth) / sf.fpx;
  const double Y = ((py - H / 2.0) * depth) / sf.fpx;
  const double Z = -depth;
  const double wind = block_wind(c, sf.wind_sigma);
  const double t = sf.exposure_s;
  double vx = wind, vz = sf.speed_mps;
  if constexpr (WIND) { vx = wind + wx; vz = sf.speed_mps + wz; }
  const double X2 = X + vx * t;
  const double Y2 = Y - terminal_velocity(D) * t;
  const double Z2 = Z + vz * t;
  p.wp1[0] = X; p.wp1[1] = Y; p.wp1[2] = Z;
  p.wp2[0] = X2; p.wp2[1] = Y2; p.wp2[2] = Z2;
  p.wd = wd;
  p.ip1[0] = px; p.ip1[1] = py;
  p.iw1 = (wd * sf.fpx) / depth;
  project(sf, X2, Y2, rr::dmax(-Z2, 0.05), wd, p.ip2, p.iw2);
  if (pick_word) *pick_word = b[2];
}

// ---- the FIELD model (rr_set_particle_model, tools/particles.py make_field_particles): a persistent particle field ----
// sf.n_particles is the run's number of particle SLOTS and sf.frame the TIME index k (t = k / cam_hz).  Slot j has a
// diameter D and a phase for good (block (j, 0, 0, 1)); it lives in the axis-aligned box that bounds its frustum (half
// sides bx = hx z_max, by = hy z_max, depth 0 .. z_max) and falls through it once every T = 2 by / v(D) seconds.  The
// number of completed falls g = floor(t / T + phase) is a word of the counter of the life's own draws (blocks
// (j, g mod 2^32, 1 | 2, 2 + g / 2^32): lateral start, start depth, wind), so every life of a slot is a new drop; the
// fractional part is its age.  Inside a life the position is the start moved by velocity x elapsed time, modulo the box
// on the two lateral axes: a translation of a uniform law, hence uniform in the box at every t; what lies outside the
// (margin-enlarged) frustum is culled (two slots in three).  Everything is a function of (key, j, k) and the settings.
// The field and the rig model share slot_draw and slot_fall; they differ in the box, the drift in depth and the placement.

// the counter of block `block` of slot j's life g: (j, g mod 2^32, block, 2 + g / 2^32)
RR_HD void life_counter(uint32_t j, double life, uint32_t block, uint32_t out[4]) {
  const double g_hi = floor(life * (1.0 / 4294967296.0)), g_lo = life - g_hi * 4294967296.0;
  out[0] = j; out[1] = (uint32_t)g_lo; out[2] = block; out[3] = 2u + (uint32_t)g_hi;
}

struct SlotDraw {                 // what slot j is for good: Philox block (j, 0, 0, 1)
  double D, phase;                // diameter (mm), phase of the fall in [0, 1)
  double wd, z_max;               // diameter (m), farthest depth shown
};
RR_HD SlotDraw slot_draw(const rr_sim_frame& sf, const double* dgrid, const double* cdf, int n_grid, uint32_t j) {
  uint32_t a[4] = {j, 0u, 0u, 1u};
  philox4x32_10(a, sf.key0, sf.key1);
  SlotDraw s;
  s.D = sample_diameter(dgrid, cdf, n_grid, unit32(a[0]));
  s.phase = unit32(a[1]);
  s.wd = s.D * 1e-3;
  s.z_max = slot_z_max(sf, s.wd);
  return s;
}

// ---- GUSTS (rr_set_particle_gusts, tools/particles.py gusts=): a wind that changes over time, field and rig models ----
// The series is a table G[0 .. n] of (x, z) metres: row i is the air's horizontal displacement at time index frame0 + i, linear
// in between; the host makes it, the statements look up, interpolate and add.  GUST is a compile-time switch of the field and rig
// generators, instantiated with WIND = true only (the gust path forms both mean-wind additions, also for a mean of (0, 0)).  With
// m = frame - frame0 (0 <= m < n, the host's check) and back = tau cam_hz the frames since the life's birth:
//   sb = m - back;  i = max(floor(sb), 0);  Gb = G[i] + (sb - i) (G[i + 1] - G[i])      the air at the drop's birth
//   dG = G[m] - Gb                                   the air's displacement over the drop's life so far
//   ge = (G[m + 1] - G[m]) cam_hz                    the air's velocity during this frame's interval
// (sb < 0: the first interval's velocity is held).  dG joins v tau in the position of a life, ge joins v in the streak's end.
// GUST = false is every function as it was: no GustFrame is read, no field of it exists in a caller's registers.
struct alignas(16) GustRow { double x, z; };   // one row of the table: 16 bytes, one load
struct GustFrame {                // what a frame's generators get of the series: wave-uniform
  const GustRow* tab;             // G[0 .. n]; never written by a kernel
  int32_t n;                      // intervals
  double m;                       // frame - frame0: an exact integer, 0 <= m < n
  GustRow gm, gm1;                // G[m], G[m + 1]
};
// the frame's part, from the table itself (the host build; a kernel fills the same fields through its scalar path)
RR_HD GustFrame gust_frame(const double* tab, int32_t n, uint32_t frame0, uint32_t frame) {
  GustFrame g;
  g.tab = reinterpret_cast<const GustRow*>(tab);
  g.n = n;
  const uint32_t mi = frame - frame0;
  g.m = (double)mi;
  g.gm = g.tab[mi];
  g.gm1 = g.tab[mi + 1];
  return g;
}
struct GustBirth {                // the two rows around a life's birth and the fraction between them: per lane
  GustRow g0, g1;
  double fr;
};
// the look-up: issued as soon as tau is known, before the life's Philox blocks, so that those cover its latency.  The index is an
// exact integer in 0 .. m <= n - 1; the comparison keeps any other value (a NaN from settings nobody checked) inside the table.
RR_HD void gust_birth(const GustFrame& gf, double cam_hz, double tau, GustBirth& gb) {
  const double back = tau * cam_hz;
  const double sb = gf.m - back;
  const double i = rr::dmax(floor(sb), 0.0);
  const int32_t ii = i < (double)gf.n ? (int32_t)i : gf.n - 1;
  gb.fr = sb - i;
  gb.g0 = gf.tab[ii];
  gb.g1 = gf.tab[ii + 1];
}
// (dGx, dGz) and (gex, gez)
RR_HD void gust_terms(const GustFrame& gf, double cam_hz, const GustBirth& gb, double dG[2], double ge[2]) {
  const double bx = gb.g0.x + gb.fr * (gb.g1.x - gb.g0.x);
  const double bz = gb.g0.z + gb.fr * (gb.g1.z - gb.g0.z);
  dG[0] = gf.gm.x - bx;
  dG[1] = gf.gm.z - bz;
  ge[0] = (gf.gm1.x - gf.gm.x) * cam_hz;
  ge[1] = (gf.gm1.z - gf.gm.z) * cam_hz;
}

// ---- SHOWERS (rr_set_particle_rate_series, tools/particles.py rate_series=): a rain rate that changes over time, field and rig ----
// Slots and tables are drawn once for the series' PEAK rate; a life is kept with the probability N(D; R) / N(D; R_peak) =
// exp(-(Lambda(R) - Lambda(R_peak)) D) of the rate R at the life's BIRTH: Marshall-Palmer thinned to the lower rate, and a drop
// that has started to fall keeps falling.  The host makes the table L[0 .. n] = min(Lambda(rate[i]) - Lambda(peak), 100) mm^-1
// (row i at time index frame0 + i, linear in between) and lays it out as n rows (L[i], L[i + 1]): 16 bytes, one load per lane.
// With m = frame - frame0 (0 <= m < n, the host's check), every step one IEEE double operation:
//   sb = max(m - tau cam_hz, 0);  i = floor(sb);  Lb = L[i] + (sb - i) (L[i + 1] - L[i]);  p = det_exp(-(Lb D))
//   alive = unit32(b[3]) < p                         b[3]: word 3 of the life's block 1, which nothing else reads
// (before the series starts its first value is held).  Lb = 0 gives p = 1.0 exactly and every life alive: a series at its peak
// leaves the records of no series.  Lb = 100 gives p <= 1.9e-22 < unit32's smallest value: no new drop.  A life that is not alive
// is culled like a slot outside the frustum.  RATE = false is every function as it was: no RateFrame is read.
struct alignas(16) RateRow { double l0, l1; };  // (L[i], L[i + 1]): 16 bytes, one load
struct RateFrame {                // what a frame's generators get of the series: wave-uniform
  const RateRow* tab;             // rows 0 .. n - 1; never written by a kernel
  int32_t n;                      // intervals
  double m;                       // frame - frame0: an exact integer, 0 <= m < n
};
RR_HD RateFrame rate_frame(const RateRow* tab, int32_t n, uint32_t frame0, uint32_t frame) {
  RateFrame r;
  r.tab = tab;
  r.n = n;
  r.m = (double)(frame - frame0);
  return r;
}
struct RateBirth {                // the row around a life's birth and the fraction inside it: per lane
  RateRow r;
  double fr;
};
// the look-up: issued as soon as tau is known, before the life's Philox blocks, so that those cover its latency.  The index is an
// exact integer in 0 .. m <= n - 1; the comparison keeps any other value (a NaN from settings nobody checked) inside the table.
RR_HD void rate_birth(const RateFrame& rf, double cam_hz, double tau, RateBirth& rb) {
  const double back = tau * cam_hz;
  const double sb = rr::dmax(rf.m - back, 0.0);
  const double i = floor(sb);
  const int32_t ii = i < (double)rf.n ? (int32_t)i : rf.n - 1;
  rb.fr = sb - i;
  rb.r = rf.tab[ii];
}
// whether the life is kept: D in mm, w = word 3 of the life's block 1
RR_HD bool rate_alive(const RateBirth& rb, double D, uint32_t w) {
  const double Lb = rb.r.l0 + rb.fr * (rb.r.l1 - rb.r.l0);
  return unit32(w) < det_exp(-(Lb * D));
}

struct SlotFall {                 // where slot j is in its fall through a box of height wy at time index sf.frame
  double v;                       // terminal velocity, m/s
  double life, age, tau;          // completed falls g, the fraction of the current one, seconds since it began
  double wind;                    // the life's wind (block 2)
  uint32_t b[4];                  // the life's block 1: lateral start, start depth, the texture pick's word, RATE: the acceptance deviate
  bool alive;                     // RATE: whether the rate series keeps the life (true without RATE: nothing reads it)
};
template <bool GUST = false, bool RATE = false>
RR_HD SlotFall slot_fall(const rr_sim_frame& sf, double cam_hz, uint32_t j, double D, double wy, double phase, const GustFrame* gf = nullptr,
                         GustBirth* gb = nullptr, const RateFrame* rf = nullptr) {
  SlotFall f;
  f.v = terminal_velocity(D);
  const double T = wy / f.v;
  const double t = (double)sf.frame / cam_hz;
  const double s = t / T + phase;
  f.life = floor(s);
  f.age = s - f.life;
  f.tau = f.age * T;
  if constexpr (GUST) gust_birth(*gf, cam_hz, f.tau, *gb);
  RateBirth rb;
  if constexpr (RATE) rate_birth(*rf, cam_hz, f.tau, rb);
  uint32_t c[4];
  life_counter(j, f.life, 1u, f.b);
  philox4x32_10(f.b, sf.key0, sf.key1);
  // RATE: decided as soon as block 1 is there -- it covers the look-up's latency; the row, the fraction and D are dead after it
  if constexpr (RATE) f.alive = rate_alive(rb, D, f.b[3]); else f.alive = true;
  life_counter(j, f.life, 2u, c);
  philox4x32_10(c, sf.key0, sf.key1);
  f.wind = block_wind(c, sf.wind_sigma);
  return f;
}

// Returns whether the particle is inside the frustum; `life` = g; *pick_word = word 2 of the life's block 1 (texture_pick).
// RATE: a life the rate series rejects is outside: one bit joins the cull, so that a kernel skips derive_drop for it as for a slot
// outside the frustum.  (No return before the position: in k_field_particles' store passes such a branch cost 32 to 116 bytes of
// scratch per lane at four waves per SIMD)
template <bool WIND = false, bool GUST = false, bool RATE = false>
RR_HD bool make_field_particle(const rr_sim_frame& sf, double cam_hz, const double* dgrid, const double* cdf, int n_grid, uint32_t j,
                               Particle& p, double& life, uint32_t* pick_word = nullptr, double wind_x = 0.0, double wind_z = 0.0,
                               const GustFrame* gf = nullptr, const RateFrame* rf = nullptr) {
  static_assert(WIND || !GUST, "the gust path forms the mean-wind additions: GUST needs WIND");
  const SlotDraw s = slot_draw(sf, dgrid, cdf, n_grid, j);
  const double W = (double)sf.sensor_w, H = (double)sf.sensor_h;
  const double hx = ((0.5 + sf.margin) * W) / sf.fpx, hy = ((0.5 + sf.margin) * H) / sf.fpx;   // frustum half-widths at unit depth
  const double bx = hx * s.z_max, by = hy * s.z_max;
  const double wx = 2.0 * bx, wy = 2.0 * by;
  GustBirth gb;
  const SlotFall f = slot_fall<GUST, RATE>(sf, cam_hz, j, s.D, wy, s.phase, gf, &gb, rf);
  double vx = f.wind, vz = sf.speed_mps;
  if constexpr (WIND) { vx = f.wind + wind_x; vz = sf.speed_mps + wind_z; }
  double qx, qz;                                            // box coordinates in units of the box: wrapped into [0, 1)
  double ux = vx, uz = vz;                                  // the velocity of the streak's end
  if constexpr (GUST) {
    double dG[2], ge[2];
    gust_terms(*gf, cam_hz, gb, dG, ge);
    qx = unit32(f.b[0]) + (vx * f.tau + dG[0]) / wx;
    qz = unit32(f.b[1]) - (vz * f.tau + dG[1]) / s.z_max;
    ux = vx + ge[0];
    uz = vz + ge[1];
  } else {
    qx = unit32(f.b[0]) + (vx * f.tau) / wx;
    qz = unit32(f.b[1]) - (vz * f.tau) / s.z_max;
  }
  const double fx = qx - floor(qx), fz = qz - floor(qz);
  const double X = fx * wx - bx;
  const double Y = by - f.age * wy;
  const double zr = fz * s.z_max;                           // depth in the box
  const double ax = hx * zr, ay = hy * zr;
  bool inside = -ax <= X && X <= ax && -ay <= Y && Y <= ay;
  if constexpr (RATE) inside = inside && f.alive;
  const double depth = rr::dmax(zr, 0.05);
  const double Z = -depth;
  const double e = sf.exposure_s;
  const double X2 = X + ux * e;
  const double Y2 = Y - f.v * e;
  const double Z2 = Z + uz * e;
  life = f.life;
  if (pick_word) *pick_word = f.b[2];
  p.wp1[0] = X; p.wp1[1] = Y; p.wp1[2] = Z;
  p.wp2[0] = X2; p.wp2[1] = Y2; p.wp2[2] = Z2;
  p.wd = s.wd;
  project(sf, X, Y, depth, s.wd, p.ip1, p.iw1);
  project(sf, X2, Y2, rr::dmax(-Z2, 0.05), s.wd, p.ip2, p.iw2);
  return inside;
}

// ---- the RIG model (rr_set_particle_rig, tools/particles.py make_rig_particles): one field, several cameras ----
// The field model with the slot's box in the RIG frame: the square [-b, b)^2 in x and z, b = r z_max, and [-by, by) in y,
// by = r_y z_max + o_y (box = {r, r_y, o_y} from the host: the reach of all views' frusta per unit depth).  x and z wrap
// modulo 2 b: the world is that lattice.  make_rig_slot is the part no view enters -- the diameter look-up, the three
// Philox blocks, the life, the wrap -- and is evaluated ONCE per slot and instant; rig_view_particle then looks at the
// slot through one view: the lattice image nearest to the camera, turned by R, culled against the frustum.
struct RigSlot {
  double X, Y, Z;                 // position in the rig frame
  double wind, v;                 // rig-frame velocity (wind, -v, speed_mps)
  double wd, z_max;               // diameter (m), farthest depth shown (the box's half side in x and z is box[0] z_max)
  double life;
  uint32_t pick_word;             // word 2 of the life's block 1 (texture_pick): one pick for every view and frame of the life
  double vx, vz;                  // WIND only (else not written, not read): rig-frame velocity (vx, -v, vz) under the mean wind;
                                  // GUST: plus the frame's gust velocity (gex, gez) -- every view and a trajectory's end use it unchanged
};

// RATE: returns whether the slot's life is alive -- decided here, once per slot, so that every view and a trajectory agree; a
// rejected slot is kept by no view (k_rig_particles treats it as a slot beyond the chunk: no view step works on it).  Without
// RATE: true.
template <bool WIND = false, bool GUST = false, bool RATE = false>
RR_HD bool make_rig_slot(const rr_sim_frame& sf, double cam_hz, const double box[3], const double* dgrid, const double* cdf, int n_grid,
                         uint32_t j, RigSlot& q, double wx = 0.0, double wz = 0.0, const GustFrame* gf = nullptr,
                         const RateFrame* rf = nullptr) {
  static_assert(WIND || !GUST, "the gust path forms the mean-wind additions: GUST needs WIND");
  const SlotDraw s = slot_draw(sf, dgrid, cdf, n_grid, j);
  const double b = box[0] * s.z_max;
  const double by = box[1] * s.z_max + box[2];
  const double w = 2.0 * b, wy = 2.0 * by;
  GustBirth gb;
  const SlotFall f = slot_fall<GUST, RATE>(sf, cam_hz, j, s.D, wy, s.phase, gf, &gb, rf);
  double vx = f.wind, vz = sf.speed_mps;
  if constexpr (WIND) { q.vx = vx = f.wind + wx; q.vz = vz = sf.speed_mps + wz; }
  double qx, qz;
  if constexpr (GUST) {                                             // once per slot, not per view
    double dG[2], ge[2];
    gust_terms(*gf, cam_hz, gb, dG, ge);
    qx = unit32(f.b[0]) + (vx * f.tau + dG[0]) / w;
    qz = unit32(f.b[1]) + (vz * f.tau + dG[1]) / w;
    q.vx = vx + ge[0];
    q.vz = vz + ge[1];
  } else {
    qx = unit32(f.b[0]) + (vx * f.tau) / w;
    qz = unit32(f.b[1]) + (vz * f.tau) / w;                         // the vehicle's motion: drops gain +speed in z
  }
  const double fx = qx - floor(qx), fz = qz - floor(qz);
  q.X = fx * w - b;
  q.Y = by - f.age * wy;
  q.Z = fz * w - b;
  q.wind = f.wind;
  q.v = f.v;
  q.wd = s.wd;
  q.z_max = s.z_max;
  q.life = f.life;
  q.pick_word = f.b[2];
  if constexpr (RATE) return f.alive;
  return true;
}

// The START of slot q's streak as the view (R row-major rig -> camera, c the camera's centre) sees it: the lattice image nearest
// to the camera, turned by R, culled, projected; d = the wrapped offset from the camera.  Returns whether the view keeps the slot.
// The rig at rest (rig_view_particle) and the rig under a trajectory (with traj_view_end) share it; it keeps the name it had.
RR_HD bool traj_view_start(const rr_sim_frame& sf, const RigSlot& q, const double box[3], const double* R, const double* c, double d[3],
                          Particle& p) {
  const double W = (double)sf.sensor_w, H = (double)sf.sensor_h;
  const double hx = ((0.5 + sf.margin) * W) / sf.fpx, hy = ((0.5 + sf.margin) * H) / sf.fpx;
  const double b = box[0] * q.z_max, w = 2.0 * b;
  double dx = q.X - c[0], dz = q.Z - c[2];
  const double dy = q.Y - c[1];
  dx = dx - floor((dx + b) / w) * w;                      // the lattice image nearest to the camera
  dz = dz - floor((dz + b) / w) * w;
  const double xc = (R[0] * dx + R[1] * dy) + R[2] * dz;
  const double yc = (R[3] * dx + R[4] * dy) + R[5] * dz;
  const double zc = (R[6] * dx + R[7] * dy) + R[8] * dz;
  const double zr = -zc;                                    // depth along the view's axis
  const double ax = hx * zr, ay = hy * zr;
  const bool inside = zr > 0.0 && zr <= q.z_max && -ax <= xc && xc <= ax && -ay <= yc && yc <= ay;
  const double depth = rr::dmax(zr, 0.05);
  d[0] = dx; d[1] = dy; d[2] = dz;
  p.wp1[0] = xc; p.wp1[1] = yc; p.wp1[2] = -depth;
  p.wd = q.wd;
  project(sf, xc, yc, depth, q.wd, p.ip1, p.iw1);
  return inside;
}
// The END of the streak: the offset e from the camera at the end of the exposure, turned by R and projected.
RR_HD void rig_view_end(const rr_sim_frame& sf, const RigSlot& q, double ex, double ey, double ez, const double* R, Particle& p) {
  const double X2 = (R[0] * ex + R[1] * ey) + R[2] * ez;
  const double Y2 = (R[3] * ex + R[4] * ey) + R[5] * ez;
  const double Z2 = (R[6] * ex + R[7] * ey) + R[8] * ez;
  p.wp2[0] = X2; p.wp2[1] = Y2; p.wp2[2] = Z2;
  project(sf, X2, Y2, rr::dmax(-Z2, 0.05), q.wd, p.ip2, p.iw2);
}
// slot q through a view at rest: the start moved by the drop's velocity x exposure.  (NOT traj_view_end with c1 == c0: the bits
// would agree, but the subtraction cannot be folded away and this is the path of every run without a trajectory.)
// WIND: the slot's (vx, vz) in place of (wind, speed_mps).
template <bool WIND = false>
RR_HD bool rig_view_particle(const rr_sim_frame& sf, const RigSlot& q, const double box[3], const double* R, const double* c, Particle& p) {
  double d[3];
  const bool inside = traj_view_start(sf, q, box, R, c, d, p);
  const double e = sf.exposure_s;
  if constexpr (WIND) rig_view_end(sf, q, d[0] + q.vx * e, d[1] + (-q.v) * e, d[2] + q.vz * e, R, p);
  else rig_view_end(sf, q, d[0] + q.wind * e, d[1] + (-q.v) * e, d[2] + sf.speed_mps * e, R, p);
  return inside;
}

// ---- the rig model under a TRAJECTORY (rr_set_particle_trajectory, tools/particles.py make_rig_particles view_end=) ----
// The view has one pose (R0, c0) at t_k and another (R1, c1) at t_k + exposure: the streak is the drop's path relative to a
// camera that moves and turns while the shutter is open.  traj_view_start with (R0, c0) hands on the wrapped offset d;
// traj_view_end moves d by the drop's velocity x exposure, subtracts the camera's own displacement c1 - c0 -- the same lattice
// image as the start, never wrapped again -- and turns it by R1.  With R1 == R0 and c1 == c0 the subtraction is - 0.0 and the
// pair gives rig_view_particle's bits.  Two calls, so that a kernel makes the second for the lanes the cull left only and R1, c1
// are not live across it.
template <bool WIND = false>
RR_HD void traj_view_end(const rr_sim_frame& sf, const RigSlot& q, const double d[3], const double* c0, const double* R1, const double* c1,
                         Particle& p) {
  const double e = sf.exposure_s;
  double vx = q.wind, vz = sf.speed_mps;
  if constexpr (WIND) { vx = q.vx; vz = q.vz; }
  rig_view_end(sf, q, (d[0] + vx * e) - (c1[0] - c0[0]), (d[1] + (-q.v) * e) - (c1[1] - c0[1]),
               (d[2] + vz * e) - (c1[2] - c0[2]), R1, p);
}

// ceil(sqrt(n)) of a non-negative integer, exactly (np.ceil(np.sqrt(.)) of the loader gives the same: a non-integer root
// is further from an integer than the rounding error of a correctly rounded sqrt)
RR_HD int64_t ceil_sqrt(int64_t n) {
  int64_t s = (int64_t)sqrt((double)n);
  while (s * s < n) s++;
  while (s > 0 && (s - 1) * (s - 1) >= n) s--;
  return s;
}

// cos / sin of -(theta), theta = acos(-fy / n) the angle of the streak (fx, fy) = start - end, evaluated exactly: -fy / n, -|fx| / n
RR_HD void exact_rotation(double fx, double fy, double& c, double& s) {
  const double n1 = sqrt(fx * fx + fy * fy);
  c = (fx / n1) * 0.0 + (fy / n1) * -1.0;
  s = -(fabs(fx) / n1);
}

// The loader's derived fields (DBManager.load_streaks_from_xml, bad_weather.py:208-241) and the frame filter
// (Generator.run, generator.py:413-420) for one particle; W x H is the RENDERED frame (sensor / render_scale).  Fills every
// field of `d` except tex_index; `ratio` is Streak.ratio (take_drop_texture's key).  Returns whether the streak is kept.
RR_HD bool derive_drop(const Particle& p, int render_scale, int W, int H, rr_drop& d, double& ratio) {
  const double rs = (double)render_scale;
  double sx = p.ip1[0] / rs, sy = p.ip1[1] / rs, ex = p.ip2[0] / rs, ey = p.ip2[1] / rs;
  const double w1 = p.iw1 / rs, w2 = p.iw2 / rs;
  sy = (double)H - sy;                                    // bad_weather.py:221-222
  ey = (double)H - ey;
  const double d0 = fabs(sx - ex), d1 = fabs(sy - ey);
  const double mwf = rr::dmax(w1, w2);                    // max(iw1, iw2): Python's max keeps the first on ties / NaN
  const int64_t max_width = (int64_t)mwf;                 // int(): truncation
  const double nrm = sqrt(d0 * d0 + d1 * d1);
  const double dir2y = -(d1 / nrm);
  const double cos_theta = (d0 / nrm) * 0.0 + dir2y * -1.0;
  const double actual_length = d1 / cos_theta;
  ratio = (double)max_width / actual_length;
  const int64_t x0 = (int64_t)rint(sx), y0 = (int64_t)rint(sy), x1 = (int64_t)rint(ex), y1 = (int64_t)rint(ey);   // round half to even
  const int64_t ddx = x0 - x1, ddy = y0 - y1;
  const int64_t length = ceil_sqrt(ddx * ddx + ddy * ddy);
  const int type = max_width >= 4 ? 0 : (max_width > 1 ? 1 : 2);
  d.x0 = (int32_t)x0; d.y0 = (int32_t)y0; d.x1 = (int32_t)x1; d.y1 = (int32_t)y1;
  d.max_width = (int32_t)max_width;
  d.length = (int32_t)length;
  d.type = type;
  d.tex_index = 0;
  d.iw1 = w1;
  d.iw2 = w2;
  d.wps[0] = p.wp1[0]; d.wps[1] = p.wp1[1]; d.wps[2] = p.wp1[2] * -1.0;      // bad_weather.py:223-224
  d.wpe[0] = p.wp2[0]; d.wpe[1] = p.wp2[1]; d.wpe[2] = p.wp2[2] * -1.0;
  // rotation of the streak texture (non-Big): cos / sin of -(theta) with theta = acos(-dy / n) (generator.py:138-145,163)
  // evaluated exactly (exact_rotation) over the integer positions
  if (type == 0) {
    d.rot_cos = 1.0;
    d.rot_sin = 0.0;
  } else {
    exact_rotation((double)ddx, (double)ddy, d.rot_cos, d.rot_sin);
  }
  const int64_t m = H > W ? H : W;
  const bool in_s = 0 <= x0 && x0 < W && 0 <= y0 && y0 < H, in_e = 0 <= x1 && x1 < W && 0 <= y1 && y1 < H;
  return max_width >= 1 && length >= 1 &&                                     // the loader's own test (bad_weather.py:238)
         max_width < m && length < m && (in_s || in_e);                        // generator.py:413-420
}

// ---- angular noise (--noise_std, generator.py:136-163) on a run's device-generated tables (tools/particles.py noise_step)
// the frame filter of Generator.run (generator.py:413-420) on a record's CURRENT end points (a rotated streak may leave)
RR_HD bool drop_in_frame(const rr_drop& d, int W, int H) {
  const int64_t m = H > W ? H : W;
  const bool in_s = 0 <= d.x0 && d.x0 < W && 0 <= d.y0 && d.y0 < H, in_e = 0 <= d.x1 && d.x1 < W && 0 <= d.y1 && d.y1 < H;
  return 1 <= d.max_width && d.max_width < m && 1 <= d.length && d.length < m && (in_s || in_e);
}

// numpy's legacy_gauss: the accepted polar pair (x1, x2), r2 = x1^2 + x2^2, yields f x2 now and f x1 for the next call
RR_HD double polar_factor(double r2) { return sqrt(-2.0 * rr::det_log(r2) / r2); }

// the noise angle of a non-Big drop in degrees: normal(0, noise_std) * noise_scale (generator.py:136)
RR_HD double noise_degrees(double g, double noise_std, double noise_scale) { return (0.0 + noise_std * g) * noise_scale; }

// a kept non-Big drop turned by noise_deg: rotation terms cos / sin(-(theta + noise) * pi / 180) as the angle sum of the exact
// cos / sin(-theta) = -dy / n, -|dx| / n (exact_rotation) of the end points BEFORE the turn and det_sincos(noise); the end
// points turned about their midpoint in hip_backend.pack_frame's operation order, truncated toward zero (numpy's int64 store)
RR_HD void noise_rotate(rr_drop& d, double noise_deg) {
  double sn, cn;
  rr::det_sincos(noise_deg * 0.017453292519943295, sn, cn);   // np.deg2rad: x * (pi / 180)
  const double sx = (double)d.x0, sy = (double)d.y0, ex = (double)d.x1, ey = (double)d.y1;
  double c0, s0;
  exact_rotation(sx - ex, sy - ey, c0, s0);
  d.rot_cos = c0 * cn + s0 * sn;
  d.rot_sin = s0 * cn - c0 * sn;
  const double mx = (ex + sx) / 2.0, my = (ey + sy) / 2.0;
  d.x0 = (int32_t)(int64_t)(((sx - mx) * cn - (sy - my) * sn) + mx);
  d.y0 = (int32_t)(int64_t)(((sx - mx) * sn + (sy - my) * cn) + my);
  d.x1 = (int32_t)(int64_t)(((ex - mx) * cn - (ey - my) * sn) + mx);
  d.y1 = (int32_t)(int64_t)(((ex - mx) * sn + (ey - my) * cn) + my);
}

// ---- streak jitter (rr_set_particle_jitter, tools/particles.py counter_jitter): a normal deviate of the drop's own ----
// Box-Muller on three words of the drop's Philox block 3: u1 has 53 bits in (0, 1] (every step exact), u2 = unit32(w2),
// g = sqrt(-2 det_log(u1)) cos(2 pi u2): + - * / sqrt, det_log and det_sincos only.  |g| < 8.6; u1 = 1 gives 0.
RR_HD double jitter_deviate(const uint32_t w[4]) {
  const double u1 = (((double)(w[0] >> 5) * 67108864.0 + (double)(w[1] >> 6)) + 1.0) * (1.0 / 9007199254740992.0);
  double sn, cn;
  rr::det_sincos(6.283185307179586 * unit32(w[2]), sn, cn);
  return sqrt(-2.0 * rr::det_log(u1)) * cn;
}
// Block 3 of the drop under the frame's key.  The generators read blocks 0, 1 and 2 of a counter (make_particle:
// (i, frame, 0 | 1 | 2, 0); the field and rig models: (j, 0, 0, 1) and the life's (j, g_lo, 1 | 2, 2 + g_hi)); nothing else
// reads a block 3 (life_counter).  i.i.d. model: particle i of frame sf.frame.
RR_HD double particle_jitter(const rr_sim_frame& sf, uint32_t i) {
  uint32_t w[4] = {i, sf.frame, 3u, 0u};
  philox4x32_10(w, sf.key0, sf.key1);
  return jitter_deviate(w);
}
// field and rig models: slot j in its life g -- the same tilt in every frame of the life and in every view
RR_HD double life_jitter(const rr_sim_frame& sf, uint32_t j, double life) {
  uint32_t w[4];
  life_counter(j, life, 3u, w);
  philox4x32_10(w, sf.key0, sf.key1);
  return jitter_deviate(w);
}
// a kept record turned by jitter_deg * g degrees (noise_rotate); Big drops are left alone
RR_HD void jitter_drop(rr_drop& d, double jitter_deg, double g) {
  if (d.type != 0) noise_rotate(d, jitter_deg * g);
}

// the block of ten textures take_drop_texture draws from (bad_weather.py:250-265): NaN falls through to the last one
RR_HD int texture_bucket(double ratio, const double* ratio_db) {
  int b = 4;
  for (int k = 3; k >= 0; k--)
    if (ratio < ratio_db[k]) b = k;
  return b;
}

}  // namespace rrsim
