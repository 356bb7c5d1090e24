// g++ build of the lens pass on INTERLEAVED bytes (k_lens_drops_hwc: the frame pipeline's lens stage and RR_TENSOR_U8_HWC)
// for tests/test_lens_pipeline_host.py: the RR_HD arithmetic of rr_lens.h walked with the kernel's own addressing -- one work item per
// 32 x 32 sub-tile of a box (rrlens::box_work), the sub-tile's refracted samples plus halo, the row pass, the column pass into the
// composite, a pixel's three channel results kept and stored as three adjacent bytes, pixel p's channel c at byte 3 p + c -- compiled for
// the host with -ffp-contract=off, against tools/lens.py apply_numpy through a transpose; and the byte label lens_label(A).
#include <cstring>
#include <string>
#include <vector>

#include "rainhip.h"
#include "rr_lens.h"

namespace {

constexpr int TL = rrlens::TILE;
constexpr int VW = TL + 2 * rrlens::MAX_RADIUS;

// one work item: what one workgroup of k_lens_drops_hwc does, its 1024 (thread, p) outputs visited in turn
void sub_tile(const uint8_t* img, uint8_t* dst, uint8_t* label, int H, int W, const rr_lens_drop& d, int tx, int ty, int R, const float* wt) {
  int bx0, bx1, by0, by1;
  if (!rrlens::lens_box(d, W, H, bx0, bx1, by0, by1)) return;
  const int ox = bx0 + tx * TL, oy = by0 + ty * TL;
  const int tw = rr::imin(TL, bx1 + 1 - ox), th = rr::imin(TL, by1 + 1 - oy);
  if (tx < 0 || ty < 0 || tw <= 0 || th <= 0) return;
  const int vw = tw + 2 * R, vh = th + 2 * R;
  const double cx = d.cx, cy = d.cy, rx = d.rx, ry = d.ry, mag = d.mag;
  std::vector<float> s_v((size_t)3 * VW * VW), s_r((size_t)VW * TL);
  for (int i = 0; i < vw * vh; i++) {
    const int hy = i / vw, hx = i - hy * vw;
    const int qx = rr::imin(rr::imax(ox - R + hx, 0), W - 1), qy = rr::imin(rr::imax(oy - R + hy, 0), H - 1);
    const double dx = (double)qx - cx, dy = (double)qy - cy;
    const double g = rrlens::lens_gain(rrlens::lens_rho2(dx, dy, rx, ry));
    int x0, x1, y0, y1;
    float fx, fy;
    rrlens::lens_sample_axis(cx, mag, dx, g, W, x0, x1, fx);
    rrlens::lens_sample_axis(cy, mag, dy, g, H, y0, y1, fy);
    const int64_t a00 = ((int64_t)y0 * W + x0) * 3, a01 = ((int64_t)y0 * W + x1) * 3, a10 = ((int64_t)y1 * W + x0) * 3, a11 = ((int64_t)y1 * W + x1) * 3;
    for (int c = 0; c < 3; c++)
      s_v[(size_t)c * VW * VW + hy * VW + hx] =
          rrlens::lens_bilinear((float)img[a00 + c], (float)img[a01 + c], (float)img[a10 + c], (float)img[a11 + c], fx, fy);
  }
  std::vector<float> A((size_t)TL * TL, 0.0f), rimf((size_t)TL * TL, 0.0f);
  std::vector<int64_t> pix((size_t)TL * TL, -1);
  std::vector<uint8_t> res((size_t)TL * TL * 3, 0);
  for (int idx = 0; idx < TL * TL; idx++) {
    const int x = idx & (TL - 1), y = idx >> 5;
    if (x < tw && y < th) {
      const double r2 = rrlens::lens_rho2((double)(ox + x) - cx, (double)(oy + y) - cy, rx, ry);
      A[idx] = rrlens::lens_coverage(r2, (double)d.edge);
      rimf[idx] = rrlens::lens_rim((double)d.rim, r2);
      pix[idx] = (int64_t)(oy + y) * W + (ox + x);
      if (label) label[pix[idx]] = rrlens::lens_label(A[idx]);
    }
  }
  for (int c = 0; c < 3; c++) {
    for (int i = 0; i < vh * TL; i++) {
      const int row = i >> 5, x = i & (TL - 1);
      if (x < tw) s_r[row * TL + x] = rrlens::lens_blur_taps(&s_v[(size_t)c * VW * VW + row * VW + x], 1, wt, R);
    }
    for (int idx = 0; idx < TL * TL; idx++) {
      if (pix[idx] < 0 || A[idx] == 0.0f) continue;
      const int x = idx & (TL - 1), y = idx >> 5;
      const float B = rrlens::lens_blur_taps(&s_r[y * TL + x], TL, wt, R);
      res[(size_t)idx * 3 + c] = rrlens::lens_round_u8(rrlens::lens_composite(A[idx], rimf[idx], B, (float)img[pix[idx] * 3 + c]));
    }
  }
  for (int idx = 0; idx < TL * TL; idx++) {
    if (pix[idx] < 0 || A[idx] == 0.0f) continue;
    uint8_t* o = dst + pix[idx] * 3;
    o[0] = res[(size_t)idx * 3 + 0]; o[1] = res[(size_t)idx * 3 + 1]; o[2] = res[(size_t)idx * 3 + 2];
  }
}

}  // namespace

extern "C" {

// the lens stage on host arrays: images / out interleaved [n][H][W][3] bytes, label [n][H][W] bytes or NULL.  -1: a table the library refuses.
int32_t rr_emu_lens_hwc_apply(int32_t n, int32_t H, int32_t W, const uint8_t* images, uint8_t* out, uint8_t* label, const int32_t* counts,
                              const rr_lens_drop* drops, int32_t cap, int32_t n_classes, const int32_t* class_radius, const float* weights) {
  if (!rrlens::check_classes(n_classes, class_radius, weights).empty()) return -1;
  const size_t px = (size_t)H * W;
  std::vector<rrlens::Box> boxes;
  std::vector<rrlens::WorkItem> work;
  std::vector<rr_lens_drop> recs;
  for (int f = 0; f < n; f++) {
    boxes.clear();
    const rr_lens_drop* fd = drops + (size_t)f * cap;
    if (!rrlens::check_frame(fd, counts[f], cap, n_classes, W, H, boxes).empty()) return -1;
    for (const rrlens::Box& b : boxes) {
      rrlens::box_work(b, f, (int32_t)recs.size(), work);
      recs.push_back(fd[b.drop]);
    }
  }
  memcpy(out, images, (size_t)n * 3 * px);
  if (label) memset(label, 0, (size_t)n * px);
  for (const rrlens::WorkItem& w : work) {
    const rr_lens_drop& d = recs[(size_t)w.drop];
    const int cls = rr::imin(rr::imax((int)d.sigma_class, 0), rrlens::MAX_CLASSES - 1);
    const int R = rr::imin(rr::imax(class_radius[cls], 0), rrlens::MAX_RADIUS);
    sub_tile(images + (size_t)w.frame * 3 * px, out + (size_t)w.frame * 3 * px, label ? label + (size_t)w.frame * px : nullptr, H, W, d, w.tx, w.ty, R,
             weights + cls * rrlens::TAPS);
  }
  return 0;
}

}  // extern "C"
