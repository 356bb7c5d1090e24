// g++ build of the per-drop streak jitter the device runs (rr_set_particle_jitter: rr_particles.h particle_jitter / life_jitter,
// jitter_deviate and noise_rotate behind derive_drop and the texture terms, as k_particles<., true>, k_field_particles<false, ., true>
// and k_rig_particles<false, ., true> chain them), for tests/test_particle_jitter_host.py: the same RR_HD code, compiled for the
// host with -ffp-contract=off, against its numpy statement in rain-rendering_amd/tools/particles.py (counter_jitter,
// expected_records(jitter=)).
#include "rainhip.h"
#include "rr_particles.h"

extern "C" {

// the deviate of n drops: block (pid[k], frame, 3, 0), or with life != NULL the life's block (pid[k], g_lo, 3, 2 + g_hi)
void rr_emu_jitter_deviates(const rr_sim_frame* sf, int32_t n, const uint32_t* pid, const double* life, double* g) {
  for (int32_t k = 0; k < n; k++) g[k] = life ? rrsim::life_jitter(*sf, pid[k], life[k]) : rrsim::particle_jitter(*sf, pid[k]);
}

// The finished records of one frame as the JIT kernels leave them, tex_index as in counter mode (counter != 0) or the first
// texture of the block of ten, which is what the stream mode's particle kernel leaves for k_particle_draws.  model:
// RR_PARTICLES_*; cam_hz for the field and rig models; view / box for the rig model.  g_out (may be NULL): the deviate of every
// kept record (0 for Big drops, which make none).  Returns the number kept (at most cap are stored).
int32_t rr_emu_jitter_records(int32_t model, int32_t counter, double jitter_deg, const rr_sim_frame* sf, double cam_hz, const rr_rig_view* view,
                              const double* box, const double* dgrid, const double* cdf, int32_t n_grid, int32_t H, int32_t W,
                              const double* ratio_db, rr_drop* out, double* g_out, int32_t cap) {
  int32_t n = 0;
  for (int32_t j = 0; j < sf->n_particles; j++) {
    rrsim::Particle p;
    uint32_t w = 0;
    double life = 0.0;
    if (model == RR_PARTICLES_RIG) {
      rrsim::RigSlot q;
      rrsim::make_rig_slot(*sf, cam_hz, box, dgrid, cdf, n_grid, (uint32_t)j, q);
      w = q.pick_word;
      life = q.life;
      if (counter) q.z_max = rr::dmin((q.wd * sf->fpx) / sf->min_px, sf->z_far);   // k_rig_particles<., true, .> forms it again per view step
      if (!rrsim::rig_view_particle(*sf, q, box, view->R, view->c, p)) continue;
    } else if (model == RR_PARTICLES_FIELD) {
      if (!rrsim::make_field_particle(*sf, cam_hz, dgrid, cdf, n_grid, (uint32_t)j, p, life, &w)) continue;
    } else {
      rrsim::make_particle(*sf, dgrid, cdf, n_grid, (uint32_t)j, p, &w);
    }
    rr_drop d;
    double ratio;
    if (!rrsim::derive_drop(p, sf->render_scale, W, H, d, ratio)) continue;
    d.tex_index = 10 * rrsim::texture_bucket(ratio, ratio_db) + (counter ? rrsim::texture_pick(w) : 0);
    double g = 0.0;
    if (d.type != 0) {
      g = model == RR_PARTICLES_IID ? rrsim::particle_jitter(*sf, (uint32_t)j) : rrsim::life_jitter(*sf, (uint32_t)j, life);
      rrsim::noise_rotate(d, jitter_deg * g);
    }
    if (n < cap) {
      out[n] = d;
      if (g_out) g_out[n] = g;
    }
    n++;
  }
  return n;
}

}  // extern "C"
