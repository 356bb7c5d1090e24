// g++ build of the lens pass (rr_lens_drops_device) for tests/test_lens_host.py: the RR_HD arithmetic of rr_lens.h that
// k_lens_drops runs on the device, chained the way the kernel chains it (refracted samples of a box plus its halo, row pass, column
// pass into the composite), compiled for the host with -ffp-contract=off, against its numpy statement in
// rain-rendering_amd/tools/lens.py (apply_numpy); and the checks the library makes of a batch before it enqueues anything.
#include <cstring>
#include <string>
#include <vector>

#include "rainhip.h"
#include "rr_lens.h"

namespace {

template <class T>
void apply_drop(const T* img, T* out, float* alpha, int H, int W, const rr_lens_drop& d, int R, const float* w) {
  int bx0, bx1, by0, by1;
  if (!rrlens::lens_box(d, W, H, bx0, bx1, by0, by1)) return;
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1, vw = bw + 2 * R, vh = bh + 2 * R;
  const double cx = d.cx, cy = d.cy, rx = d.rx, ry = d.ry, mag = d.mag;
  const int64_t plane = (int64_t)H * W;
  std::vector<float> v((size_t)3 * vw * vh), r((size_t)bw * vh);
  for (int hy = 0; hy < vh; hy++)
    for (int hx = 0; hx < vw; hx++) {
      const int qx = rr::imin(rr::imax(bx0 - R + hx, 0), W - 1), qy = rr::imin(rr::imax(by0 - R + hy, 0), H - 1);
      const double dx = (double)qx - cx, dy = (double)qy - cy;
      const double g = rrlens::lens_gain(rrlens::lens_rho2(dx, dy, rx, ry));
      int x0, x1, y0, y1;
      float fx, fy;
      rrlens::lens_sample_axis(cx, mag, dx, g, W, x0, x1, fx);
      rrlens::lens_sample_axis(cy, mag, dy, g, H, y0, y1, fy);
      for (int c = 0; c < 3; c++) v[((size_t)c * vh + hy) * vw + hx] = rrlens::lens_refract(img + c * plane, W, y0, y1, x0, x1, fx, fy);
    }
  for (int c = 0; c < 3; c++) {
    for (int row = 0; row < vh; row++)
      for (int x = 0; x < bw; x++) r[(size_t)row * bw + x] = rrlens::lens_blur_taps(&v[((size_t)c * vh + row) * vw + x], 1, w, R);
    for (int y = 0; y < bh; y++)
      for (int x = 0; x < bw; x++) {
        const double r2 = rrlens::lens_rho2((double)(bx0 + x) - cx, (double)(by0 + y) - cy, rx, ry);
        const float A = rrlens::lens_coverage(r2, (double)d.edge);
        const int64_t pix = (int64_t)(by0 + y) * W + (bx0 + x);
        if (alpha) alpha[pix] = A;
        if (A == 0.0f) continue;
        const float B = rrlens::lens_blur_taps(&r[(size_t)y * bw + x], bw, w, R);
        out[c * plane + pix] = rrlens::lens_store(rrlens::lens_composite(A, rrlens::lens_rim((double)d.rim, r2), B, (float)img[c * plane + pix]),
                                                  static_cast<T*>(nullptr));
      }
  }
}

std::string check(int32_t n, int32_t H, int32_t W, const int32_t* counts, const rr_lens_drop* drops, int32_t cap, int32_t n_classes,
                  const int32_t* class_radius, const float* weights, int64_t* n_work) {
  std::string why = rrlens::check_classes(n_classes, class_radius, weights);
  if (!why.empty()) return "blur table: " + why;
  std::vector<rrlens::Box> boxes;
  std::vector<rrlens::WorkItem> work;
  for (int f = 0; f < n; f++) {
    boxes.clear();
    why = rrlens::check_frame(drops + (size_t)f * cap, counts[f], cap, n_classes, W, H, boxes);
    if (!why.empty()) return "frame " + std::to_string(f) + ": " + why;
    for (const rrlens::Box& b : boxes) rrlens::box_work(b, f, b.drop, work);
  }
  if (n_work) *n_work = (int64_t)work.size();
  return "";
}

}  // namespace

extern "C" {

// the library's checks of a batch's tables: 0, or -1 with the reason in msg; n_work: the work items the call would upload
int32_t rr_emu_lens_check(int32_t n, int32_t H, int32_t W, const int32_t* counts, const rr_lens_drop* drops, int32_t cap, int32_t n_classes,
                          const int32_t* class_radius, const float* weights, char* msg, int32_t msg_cap, int64_t* n_work) {
  const std::string why = check(n, H, W, counts, drops, cap, n_classes, class_radius, weights, n_work);
  if (msg && msg_cap > 0) {
    strncpy(msg, why.c_str(), (size_t)msg_cap - 1);
    msg[msg_cap - 1] = 0;
  }
  return why.empty() ? 0 : -1;
}

// the lens pass on host arrays: images / out planar [n][3][H][W] (dtype RR_TENSOR_*), alpha [n][H][W] or NULL
int32_t rr_emu_lens_apply(int32_t n, int32_t H, int32_t W, int32_t dtype, const void* images, void* out, float* alpha, const int32_t* counts,
                          const rr_lens_drop* drops, int32_t cap, int32_t n_classes, const int32_t* class_radius, const float* weights) {
  if (!check(n, H, W, counts, drops, cap, n_classes, class_radius, weights, nullptr).empty()) return -1;
  const size_t px = (size_t)H * W, el = dtype == RR_TENSOR_F32 ? 4 : 1;
  memcpy(out, images, (size_t)n * 3 * px * el);
  if (alpha) memset(alpha, 0, (size_t)n * px * sizeof(float));
  for (int f = 0; f < n; f++)
    for (int i = 0; i < counts[f]; i++) {
      const rr_lens_drop& d = drops[(size_t)f * cap + i];
      const int cls = (int)d.sigma_class, R = class_radius[cls];
      const float* w = weights + cls * rrlens::TAPS;
      float* al = alpha ? alpha + (size_t)f * px : nullptr;
      if (dtype == RR_TENSOR_F32)
        apply_drop(static_cast<const float*>(images) + (size_t)f * 3 * px, static_cast<float*>(out) + (size_t)f * 3 * px, al, H, W, d, R, w);
      else
        apply_drop(static_cast<const uint8_t*>(images) + (size_t)f * 3 * px, static_cast<uint8_t*>(out) + (size_t)f * 3 * px, al, H, W, d, R, w);
    }
  return 0;
}

}  // extern "C"
