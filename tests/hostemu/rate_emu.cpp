// g++ build of the field and rig generators under a rate series, as the device runs them (rr_set_particle_rate_series:
// rr_particles.h rate_frame, make_field_particle<WIND, GUST, true>, make_rig_slot<WIND, GUST, true> + rig_view_particle<WIND> or
// traj_view_start + traj_view_end<WIND>, then derive_drop, the texture terms and the jitter as the RATE instantiations of
// k_field_particles and k_rig_particles chain them), for tests/test_particle_showers_host.py: the same RR_HD code, compiled for
// the host with -ffp-contract=off, against its numpy statement in rain-rendering_amd/tools/particles.py (rate_series=).
#include <vector>

#include "rainhip.h"
#include "rr_particles.h"

namespace {

struct Air {                       // rr_set_particle_wind's and rr_set_particle_gusts' arguments (gn == 0: no gust series)
  int32_t wind;                    // whether the mean-wind additions are formed (the library: a non-zero mean, or a gust series)
  double wx, wz;
  int32_t gn;
  uint32_t gframe0;
  const double* disp;
};

// the table as rr_set_particle_rate_series lays it out: rows (L[i], L[i + 1])
std::vector<rrsim::RateRow> rate_rows(int32_t n, const double* dlam) {
  std::vector<rrsim::RateRow> rows((size_t)n);
  for (int32_t i = 0; i < n; i++) rows[(size_t)i] = rrsim::RateRow{dlam[i], dlam[i + 1]};
  return rows;
}

template <bool WIND, bool GUST>
bool rate_particle_as(int32_t model, const rr_sim_frame& sf, double cam_hz, const rr_rig_view* view, const rr_traj_pose* pose, const double* box,
                      const double* dgrid, const double* cdf, int32_t n_grid, uint32_t j, const Air& air, const rrsim::GustFrame* gf,
                      const rrsim::RateFrame& rf, int32_t counter, rrsim::Particle& p, double& life, uint32_t& w) {
  if (model == RR_PARTICLES_RIG) {
    rrsim::RigSlot q;
    const bool alive = rrsim::make_rig_slot<WIND, GUST, true>(sf, cam_hz, box, dgrid, cdf, n_grid, j, q, air.wx, air.wz, gf, &rf);
    w = q.pick_word;
    life = q.life;
    if (counter) q.z_max = rr::dmin((q.wd * sf.fpx) / sf.min_px, sf.z_far);   // k_rig_particles<., true, ...> forms it again per view step
    if (pose) {
      double d[3];
      const bool inside = rrsim::traj_view_start(sf, q, box, pose->R0, pose->c0, d, p);
      rrsim::traj_view_end<WIND>(sf, q, d, pose->c0, pose->R1, pose->c1, p);
      return alive && inside;
    }
    return rrsim::rig_view_particle<WIND>(sf, q, box, view->R, view->c, p) && alive;
  }
  return rrsim::make_field_particle<WIND, GUST, true>(sf, cam_hz, dgrid, cdf, n_grid, j, p, life, &w, air.wx, air.wz, gf, &rf);
}

// slot j of the frame under (model, view | pose, air, series): whether the model keeps it; its life and pick word
bool rate_particle(int32_t model, const rr_sim_frame& sf, double cam_hz, const rr_rig_view* view, const rr_traj_pose* pose, const double* box,
                   const double* dgrid, const double* cdf, int32_t n_grid, uint32_t j, const Air& air, const rrsim::RateFrame& rf,
                   int32_t counter, rrsim::Particle& p, double& life, uint32_t& w) {
  if (air.gn > 0) {
    const rrsim::GustFrame gf = rrsim::gust_frame(air.disp, air.gn, air.gframe0, sf.frame);
    return rate_particle_as<true, true>(model, sf, cam_hz, view, pose, box, dgrid, cdf, n_grid, j, air, &gf, rf, counter, p, life, w);
  }
  if (air.wind) return rate_particle_as<true, false>(model, sf, cam_hz, view, pose, box, dgrid, cdf, n_grid, j, air, nullptr, rf, counter, p, life, w);
  return rate_particle_as<false, false>(model, sf, cam_hz, view, pose, box, dgrid, cdf, n_grid, j, air, nullptr, rf, counter, p, life, w);
}

}  // namespace

extern "C" {

// every slot of one frame: 13 doubles each (wp1, wp2, wd, ip1, ip2, iw1, iw2), whether the model keeps it, its life
void rr_emu_rate_particles(int32_t model, int32_t wind, double wx, double wz, int32_t gn, uint32_t gframe0, const double* disp, int32_t rn,
                           uint32_t rframe0, const double* dlam, const rr_sim_frame* sf, double cam_hz, const rr_rig_view* view,
                           const rr_traj_pose* pose, const double* box, const double* dgrid, const double* cdf, int32_t n_grid, double* out,
                           uint8_t* inside, double* life) {
  const Air air{wind, wx, wz, gn, gframe0, disp};
  const std::vector<rrsim::RateRow> rows = rate_rows(rn, dlam);
  const rrsim::RateFrame rf = rrsim::rate_frame(rows.data(), rn, rframe0, sf->frame);
  for (int32_t j = 0; j < sf->n_particles; j++) {
    rrsim::Particle p;
    uint32_t w;
    inside[j] = rate_particle(model, *sf, cam_hz, view, pose, box, dgrid, cdf, n_grid, (uint32_t)j, air, rf, 0, p, life[j], w) ? 1 : 0;
    double* o = out + 13 * (int64_t)j;
    for (int k = 0; k < 3; k++) o[k] = p.wp1[k], o[3 + k] = p.wp2[k];
    o[6] = p.wd;
    o[7] = p.ip1[0]; o[8] = p.ip1[1]; o[9] = p.ip2[0]; o[10] = p.ip2[1];
    o[11] = p.iw1; o[12] = p.iw2;
  }
}

// The finished records of one frame as the RATE kernels leave them: tex_index as in counter mode (counter != 0) or the first
// texture of the block of ten, which is what the stream mode's particle kernel leaves for k_particle_draws; jitter_deg != 0: the JIT
// instantiation.  Returns the number kept (at most cap are stored).
int32_t rr_emu_rate_records(int32_t model, int32_t counter, double jitter_deg, int32_t wind, double wx, double wz, int32_t gn, uint32_t gframe0,
                            const double* disp, int32_t rn, uint32_t rframe0, const double* dlam, const rr_sim_frame* sf, double cam_hz,
                            const rr_rig_view* view, const rr_traj_pose* pose, const double* box, const double* dgrid, const double* cdf,
                            int32_t n_grid, int32_t H, int32_t W, const double* ratio_db, rr_drop* out, int32_t cap) {
  const Air air{wind, wx, wz, gn, gframe0, disp};
  const std::vector<rrsim::RateRow> rows = rate_rows(rn, dlam);
  const rrsim::RateFrame rf = rrsim::rate_frame(rows.data(), rn, rframe0, sf->frame);
  int32_t n = 0;
  for (int32_t j = 0; j < sf->n_particles; j++) {
    rrsim::Particle p;
    uint32_t w = 0;
    double life;
    if (!rate_particle(model, *sf, cam_hz, view, pose, box, dgrid, cdf, n_grid, (uint32_t)j, air, rf, counter, p, life, w)) continue;
    rr_drop d;
    double ratio;
    if (!rrsim::derive_drop(p, sf->render_scale, W, H, d, ratio)) continue;
    d.tex_index = 10 * rrsim::texture_bucket(ratio, ratio_db) + (counter ? rrsim::texture_pick(w) : 0);
    if (jitter_deg != 0.0 && d.type != 0) rrsim::noise_rotate(d, jitter_deg * rrsim::life_jitter(*sf, (uint32_t)j, life));
    if (n < cap) out[n] = d;
    n++;
  }
  return n;
}

}  // extern "C"
