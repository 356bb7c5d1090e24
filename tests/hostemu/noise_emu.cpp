// g++ build of the angular-noise arithmetic the device runs (rr_device.h det_log / det_sincos, rr_particles.h polar_factor /
// noise_degrees / noise_rotate), for tests/test_particle_noise_host.py: the same RR_HD code as k_noise_chains, compiled for
// the host with -ffp-contract=off, against its numpy statement in rain-rendering_amd/tools/particles.py.
#include "rainhip.h"
#include "rr_particles.h"

extern "C" {

void rr_emu_det_log(int64_t n, const double* x, double* out) {
  for (int64_t i = 0; i < n; i++) out[i] = rr::det_log(x[i]);
}

void rr_emu_det_sincos(int64_t n, const double* x, double* sn, double* cn) {
  for (int64_t i = 0; i < n; i++) rr::det_sincos(x[i], sn[i], cn[i]);
}

void rr_emu_polar_factor(int64_t n, const double* r2, double* out) {
  for (int64_t i = 0; i < n; i++) out[i] = rrsim::polar_factor(r2[i]);
}

// records in place: rotation terms and turned end points of every record (Big or not) by noise_degrees(g[i], ...)
void rr_emu_noise_rotate(int64_t n, rr_drop* recs, const double* g, double noise_std, double noise_scale) {
  for (int64_t i = 0; i < n; i++) rrsim::noise_rotate(recs[i], rrsim::noise_degrees(g[i], noise_std, noise_scale));
}

int rr_emu_drop_in_frame(const rr_drop* d, int32_t W, int32_t H) { return rrsim::drop_in_frame(*d, W, H) ? 1 : 0; }

}  // extern "C"
