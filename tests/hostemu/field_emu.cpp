// g++ build of the field particle model the device runs (rr_particles.h make_field_particle, then derive_drop and
// texture_bucket as k_field_particles chains them), for tests/test_particle_field_host.py: the same RR_HD code, compiled
// for the host with -ffp-contract=off, against its numpy statement in rain-rendering_amd/tools/particles.py.
#include "rainhip.h"
#include "rr_particles.h"

extern "C" {

// every slot of one frame: 15 doubles per slot (wp1, wp2, wd, ip1, ip2, iw1, iw2), whether it is inside the frustum, its life
void rr_emu_field_particles(const rr_sim_frame* sf, double cam_hz, const double* dgrid, const double* cdf, int32_t n_grid,
                            double* out, uint8_t* inside, double* life) {
  for (int32_t j = 0; j < sf->n_particles; j++) {
    rrsim::Particle p;
    inside[j] = rrsim::make_field_particle(*sf, cam_hz, dgrid, cdf, n_grid, (uint32_t)j, p, life[j]) ? 1 : 0;
    double* o = out + 15 * (int64_t)j;
    for (int k = 0; k < 3; k++) o[k] = p.wp1[k], o[3 + k] = p.wp2[k];
    o[6] = p.wd;
    o[7] = p.ip1[0]; o[8] = p.ip1[1]; o[9] = p.ip2[0]; o[10] = p.ip2[1];
    o[11] = p.iw1; o[12] = p.iw2;
    o[13] = 0.0; o[14] = 0.0;
  }
}

// the frame's records in slot order as the kernel leaves them in front of the draws: tex_index = first texture of the
// drop's block of ten.  Returns the number kept (at most cap are stored).
int32_t rr_emu_field_records(const rr_sim_frame* sf, double cam_hz, const double* dgrid, const double* cdf, int32_t n_grid,
                             int32_t H, int32_t W, const double* ratio_db, rr_drop* out, int32_t cap) {
  int32_t n = 0;
  for (int32_t j = 0; j < sf->n_particles; j++) {
    rrsim::Particle p;
    double life, ratio;
    if (!rrsim::make_field_particle(*sf, cam_hz, dgrid, cdf, n_grid, (uint32_t)j, p, life)) continue;
    rr_drop d;
    if (!rrsim::derive_drop(p, sf->render_scale, W, H, d, ratio)) continue;
    d.tex_index = 10 * rrsim::texture_bucket(ratio, ratio_db);
    if (n < cap) out[n] = d;
    n++;
  }
  return n;
}

}  // extern "C"
