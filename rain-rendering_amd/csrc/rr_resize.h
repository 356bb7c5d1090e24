// rr_resize.h -- the render-scale resize of the input files: cv2.resize(INTER_LINEAR) as the frame loader of
// Generator.run applies it to image / 255 (float64) and to the depth map (float32), stated once.
//
// The RR_HD functions are called by k_resize_in / k_resize_depth on gfx950, by rr_io_read_frames_scaled on the host (rr_png.cpp) and
// by the g++ library of the CPU tier (tests/test_input_resize_host.py), which proves them equal, bit for bit, to their numpy statement
// (common/imgops.py resize_linear).  + - * / floor only, in IEEE float64, in the order written here, no FMA contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(RR_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RR_HD __host__ __device__ inline
#else
#define RR_HD inline
#endif
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rrresize {

constexpr int MAX_SIDE = 16384;      // rr_set_input_resize: the largest source side

// s / d: the step of the source coordinate per destination index
RR_HD double resize_scale(int d, int s) { return (double)s / (double)d; }

// destination index k of an axis -> the two source indices, clamped to [0, s - 1], and the weight of the second one:
// f = (k + 0.5) * (s / d) - 0.5, weight f - floor(f), or 0 where floor(f) < 0
RR_HD void resize_coord(int k, int s, double scale, int32_t& i0, int32_t& i1, double& w) {
  const double f = ((double)k + 0.5) * scale - 0.5;
  const double fl = floor(f);
  const int64_t a = (int64_t)fl;
  w = a < 0 ? 0.0 : f - fl;
  const int64_t b = a + 1;
  i0 = (int32_t)(a < 0 ? 0 : (a > s - 1 ? s - 1 : a));
  i1 = (int32_t)(b < 0 ? 0 : (b > s - 1 ? s - 1 : b));
}

// one output sample: (a00 * (1 - wx) + a01 * wx) * (1 - wy) + (a10 * (1 - wx) + a11 * wx) * wy, numpy's order
RR_HD double resize_sample(double a00, double a01, double a10, double a11, double wx, double wy) {
  const double ux = 1 - wx, uy = 1 - wy;
  const double top = a00 * ux + a01 * wx, bot = a10 * ux + a11 * wx;
  return top * uy + bot * wy;
}

// the samples as the loader forms them: image byte / 255.0 (generator.py:352), depth sample / 256 in float32 (metres), widened
RR_HD double image_unit(uint8_t v) { return (double)v / 255.0; }
RR_HD float depth_metres(uint16_t v) { return (float)v / 256.0f; }

}  // namespace rrresize
