// rr_lens.h -- drops on the lens: the per-pixel arithmetic of rr_lens_drops_device, and the host's checks of a batch.
//
// The RR_HD functions are called by k_lens_drops on gfx950 and compiled by g++ for the CPU tier (tests/test_lens_host.py), which
// proves them equal, bit for bit, to their numpy statement in rain-rendering_amd/tools/lens.py (apply_numpy).  + - * / sqrt floor rint
// min max only, in the order written here, no FMA contraction; coordinates in double, pixel values in float.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "rainhip.h"
#include "rr_device.h"

namespace rrlens {

constexpr int MAX_CLASSES = 16;     // blur classes of a call
constexpr int MAX_RADIUS = 15;      // taps on either side of the centre
constexpr int TAPS = 2 * MAX_RADIUS + 1;
constexpr int TILE = 32;            // a work item's outputs: TILE x TILE pixels of one drop's bounding box

// the drop's bounding box clipped to the frame, inclusive: floor(c - r) .. floor(c + r) + 1; false when nothing of it is inside
RR_HD bool lens_box(const rr_lens_drop& d, int W, int H, int& x0, int& x1, int& y0, int& y1) {
  const double bx0 = rr::dmax(floor((double)d.cx - (double)d.rx), 0.0), bx1 = rr::dmin(floor((double)d.cx + (double)d.rx) + 1.0, (double)(W - 1));
  const double by0 = rr::dmax(floor((double)d.cy - (double)d.ry), 0.0), by1 = rr::dmin(floor((double)d.cy + (double)d.ry) + 1.0, (double)(H - 1));
  if (!(bx1 >= bx0 && by1 >= by0)) return false;
  x0 = (int)bx0; x1 = (int)bx1; y0 = (int)by0; y1 = (int)by1;
  return true;
}

// rho^2 = u^2 + v^2 from the offsets to the centre
RR_HD double lens_rho2(double dx, double dy, double rx, double ry) {
  const double u = dx / rx, v = dy / ry;
  return u * u + v * v;
}

// coverage A = t t (3 - 2 t), t = clamp((1 - rho^2) / edge, 0, 1)
RR_HD float lens_coverage(double r2, double edge) {
  const double t = rr::dmin(rr::dmax((1.0 - r2) / edge, 0.0), 1.0);
  return (float)(t * t * (3.0 - 2.0 * t));
}

// g = 1 / sqrt(1 - 0.75 min(rho^2, 1))
RR_HD double lens_gain(double r2) { return 1.0 / sqrt(1.0 - 0.75 * rr::dmin(r2, 1.0)); }

// the sample coordinate along one axis, clamped to the frame: c - mag dq g; its lower and upper neighbour and the fraction
RR_HD void lens_sample_axis(double c, double mag, double dq, double g, int size, int& i0, int& i1, float& f) {
  double s = c - (mag * dq) * g;
  s = rr::dmin(rr::dmax(s, 0.0), (double)(size - 1));
  const double fl = floor(s);
  f = (float)(s - fl);
  i0 = rr::imin(rr::imax((int)fl, 0), size - 1);
  i1 = rr::imin(i0 + 1, size - 1);
}

RR_HD float lens_bilinear(float p00, float p01, float p10, float p11, float fx, float fy) {
  const float top = p00 + fx * (p01 - p00);
  const float bot = p10 + fx * (p11 - p10);
  return top + fy * (bot - top);
}

// one blur pass at one output: 2 R + 1 taps `stride` elements apart, added in ascending offset order
template <class Src, class Wt>
RR_HD float lens_blur_taps(Src src, int stride, Wt w, int R) {
  float acc = w[0] * src[0];
  for (int k = 1; k <= 2 * R; k++) acc = acc + w[k] * src[k * stride];
  return acc;
}

// rim darkening 1 - rim rho^2 rho^2
RR_HD float lens_rim(double rim, double r2) { return (float)(1.0 - (rim * r2) * r2); }

// out = (1 - A) in + A (rim B)
RR_HD float lens_composite(float A, float rimf, float B, float in) { return (1.0f - A) * in + A * (rimf * B); }

// a byte tensor stores clamp(rint(out), 0, 255), half to even
RR_HD uint8_t lens_round_u8(float v) { return (uint8_t)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

// the frame pipeline's per-pixel drop label (rr_pipeline_lens.alpha_png): one float multiply, then half to even
RR_HD uint8_t lens_label(float A) { return lens_round_u8(A * 255.0f); }

RR_HD float lens_store(float v, float*) { return v; }
RR_HD uint8_t lens_store(float v, uint8_t*) { return lens_round_u8(v); }

// V(q): the input plane seen through the drop at pixel (qx, qy) of the frame
template <class Plane>
RR_HD float lens_refract(Plane img, int W, int i_y0, int i_y1, int i_x0, int i_x1, float fx, float fy) {
  const float p00 = (float)img[(int64_t)i_y0 * W + i_x0], p01 = (float)img[(int64_t)i_y0 * W + i_x1];
  const float p10 = (float)img[(int64_t)i_y1 * W + i_x0], p11 = (float)img[(int64_t)i_y1 * W + i_x1];
  return lens_bilinear(p00, p01, p10, p11, fx, fy);
}

// ---- host side: what rr_lens_drops_device checks before it enqueues anything, and the work list it uploads ----------------------
struct Box {
  int32_t x0, x1, y0, y1, drop;
};
struct WorkItem {                    // one workgroup of k_lens_drops: sub-tile (tx, ty) of drop `drop` (an index into the uploaded records)
  int32_t frame, drop, tx, ty;
};

inline bool finite_f(float v) { return v - v == 0.0f; }

// "" or the reason the blur table is refused
inline std::string check_classes(int32_t n_classes, const int32_t* class_radius, const float* weights) {
  if (n_classes < 1 || n_classes > MAX_CLASSES || !class_radius || !weights) return "n_classes outside 1 .. 16, or a null table";
  for (int c = 0; c < n_classes; c++) {
    if (class_radius[c] < 0 || class_radius[c] > MAX_RADIUS) return "class " + std::to_string(c) + ": radius outside 0 .. 15";
    for (int k = 0; k <= 2 * class_radius[c]; k++)
      if (!finite_f(weights[c * TAPS + k])) return "class " + std::to_string(c) + ": a weight that is not finite";
  }
  return "";
}

// One frame's table: "" or the reason it is refused.  The boxes inside the frame are appended to `boxes` (drop = index in the table).
// The overlap test sorts the frame's boxes by x0 and sweeps: a box is compared with its successors while they start at or before its
// right edge.
inline std::string check_frame(const rr_lens_drop* drops, int32_t count, int32_t cap, int32_t n_classes, int W, int H, std::vector<Box>& boxes) {
  if (count < 0 || count > cap || count > RR_MAX_LENS_DROPS) return "count " + std::to_string(count) + " outside 0 .. min(cap, RR_MAX_LENS_DROPS)";
  const size_t first = boxes.size();
  for (int i = 0; i < count; i++) {
    const rr_lens_drop& d = drops[i];
    const std::string at = "drop " + std::to_string(i) + ": ";
    if (!(finite_f(d.cx) && finite_f(d.cy) && finite_f(d.rx) && finite_f(d.ry) && finite_f(d.mag) && finite_f(d.edge) && finite_f(d.rim) &&
          finite_f(d.sigma_class)))
      return at + "a field that is not finite";
    if (!(d.rx > 0.0f && d.ry > 0.0f)) return at + "rx and ry must be positive";
    if (!(d.mag >= 1.0f)) return at + "mag must be at least 1";
    if (!(d.edge > 0.0f && d.edge <= 1.0f)) return at + "edge outside (0, 1]";
    if (!(d.rim >= 0.0f && d.rim <= 1.0f)) return at + "rim outside [0, 1]";
    if (!(d.sigma_class >= 0.0f && d.sigma_class < (float)n_classes && d.sigma_class == floorf(d.sigma_class))) return at + "sigma_class is not a class of the table";
    Box b;
    b.drop = i;
    if (lens_box(d, W, H, b.x0, b.x1, b.y0, b.y1)) boxes.push_back(b);
  }
  std::vector<Box> s(boxes.begin() + (std::ptrdiff_t)first, boxes.end());
  std::sort(s.begin(), s.end(), [](const Box& a, const Box& b) { return a.x0 < b.x0; });
  for (size_t i = 0; i < s.size(); i++)
    for (size_t j = i + 1; j < s.size() && s[j].x0 <= s[i].x1; j++)
      if (s[j].y0 <= s[i].y1 && s[i].y0 <= s[j].y1)
        return "the bounding boxes of drops " + std::to_string(s[i].drop) + " and " + std::to_string(s[j].drop) + " overlap";
  return "";
}

// the work items of one box
inline void box_work(const Box& b, int32_t frame, int32_t drop, std::vector<WorkItem>& work) {
  const int ntx = (b.x1 - b.x0 + TILE) / TILE, nty = (b.y1 - b.y0 + TILE) / TILE;
  for (int ty = 0; ty < nty; ty++)
    for (int tx = 0; tx < ntx; tx++) work.push_back(WorkItem{frame, drop, tx, ty});
}

}  // namespace rrlens
