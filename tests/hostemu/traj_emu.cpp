// g++ build of the rig particle model under a trajectory, as the device runs it (rr_particles.h make_rig_slot +
// traj_view_start + traj_view_end, then derive_drop and texture_bucket as k_rig_particles<.., TRAJ = true> chains them), for
// tests/test_particle_trajectory_host.py: the same RR_HD code, compiled for the host with -ffp-contract=off, against its
// numpy statement in rain-rendering_amd/tools/particles.py (make_rig_particles view_end=).
#include "rainhip.h"
#include "rr_particles.h"

extern "C" {

int32_t rr_emu_sizeof_traj_pose(void) { return (int32_t)sizeof(rr_traj_pose); }

// every slot of one instant as one view's pose sees it: 13 doubles per slot (wp1, wp2, wd, ip1, ip2, iw1, iw2), whether the
// view keeps it, its life.  The end of the streak is formed for every slot here (the kernel: for the kept ones only).
void rr_emu_traj_particles(const rr_sim_frame* sf, double cam_hz, const rr_traj_pose* pose, const double* box, const double* dgrid,
                           const double* cdf, int32_t n_grid, double* out, uint8_t* inside, double* life) {
  for (int32_t j = 0; j < sf->n_particles; j++) {
    rrsim::RigSlot q;
    rrsim::Particle p;
    double d[3];
    rrsim::make_rig_slot(*sf, cam_hz, box, dgrid, cdf, n_grid, (uint32_t)j, q);
    inside[j] = rrsim::traj_view_start(*sf, q, box, pose->R0, pose->c0, d, p) ? 1 : 0;
    rrsim::traj_view_end(*sf, q, d, pose->c0, pose->R1, pose->c1, p);
    life[j] = q.life;
    double* o = out + 13 * (int64_t)j;
    for (int k = 0; k < 3; k++) o[k] = p.wp1[k], o[3 + k] = p.wp2[k];
    o[6] = p.wd;
    o[7] = p.ip1[0]; o[8] = p.ip1[1]; o[9] = p.ip2[0]; o[10] = p.ip2[1];
    o[11] = p.iw1; o[12] = p.iw2;
  }
}

// the records of one instant's frame of one view in slot order as the kernel leaves them in front of the draws: tex_index =
// first texture of the drop's block of ten.  Returns the number kept (at most cap are stored).
int32_t rr_emu_traj_records(const rr_sim_frame* sf, double cam_hz, const rr_traj_pose* pose, const double* box, const double* dgrid,
                            const double* cdf, int32_t n_grid, int32_t H, int32_t W, const double* ratio_db, rr_drop* out, int32_t cap) {
  int32_t n = 0;
  for (int32_t j = 0; j < sf->n_particles; j++) {
    rrsim::RigSlot q;
    rrsim::Particle p;
    double d[3], ratio;
    rrsim::make_rig_slot(*sf, cam_hz, box, dgrid, cdf, n_grid, (uint32_t)j, q);
    if (!rrsim::traj_view_start(*sf, q, box, pose->R0, pose->c0, d, p)) continue;
    rrsim::traj_view_end(*sf, q, d, pose->c0, pose->R1, pose->c1, p);
    rr_drop r;
    if (!rrsim::derive_drop(p, sf->render_scale, W, H, r, ratio)) continue;
    r.tex_index = 10 * rrsim::texture_bucket(ratio, ratio_db);
    if (n < cap) out[n] = r;
    n++;
  }
  return n;
}

}  // extern "C"
