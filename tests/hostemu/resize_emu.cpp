// resize_emu.cpp -- the g++ build of csrc/rr_resize.h for the CPU tier (tests/test_input_resize_host.py): what k_resize_in /
// k_resize_depth compute per output sample, looped over a frame.  Kinds as in include/rainhip.h (RR_RESIZE_*; depth 0 / RR_DEPTH_U16).
#include <stdint.h>

#include "rainhip.h"
#include "rr_convert.h"
#include "rr_resize.h"

namespace {

// channel c (B G R) of source pixel (y, x) as the loader's float64 sample
double image_sample(const void* src, int kind, int sH, int sW, int y, int x, int c) {
  const int64_t px = (int64_t)y * sW + x, plane = (int64_t)sH * sW;
  if (kind == RR_RESIZE_BGR_U8) return rrresize::image_unit(static_cast<const uint8_t*>(src)[px * 3 + c]);
  if (kind == RR_RESIZE_RGB_U8_PLANAR) return rrresize::image_unit(static_cast<const uint8_t*>(src)[(2 - c) * plane + px]);
  if (kind == RR_RESIZE_RGB_F32_PLANAR) return (double)static_cast<const float*>(src)[(2 - c) * plane + px];
  // rr_tensor_batch's other formats: interleaved R G B, and the half types widened as the kernels widen them (csrc/rr_convert.h)
  const int64_t il = rrconv::interleaved_index(px, 2 - c), pl = rrconv::planar_index(px, 2 - c, plane);
  if (kind == RR_RESIZE_RGB_U8) return rrresize::image_unit(static_cast<const uint8_t*>(src)[il]);
  if (kind == RR_RESIZE_RGB_F32) return (double)static_cast<const float*>(src)[il];
  const uint16_t* hs = static_cast<const uint16_t*>(src);
  if (kind == RR_RESIZE_RGB_F16_PLANAR) return (double)rrconv::bits_f32(rrconv::widen_bits<0>(hs[pl]));
  if (kind == RR_RESIZE_RGB_BF16_PLANAR) return (double)rrconv::bits_f32(rrconv::widen_bits<1>(hs[pl]));
  if (kind == RR_RESIZE_RGB_F16) return (double)rrconv::bits_f32(rrconv::widen_bits<0>(hs[il]));
  return (double)rrconv::bits_f32(rrconv::widen_bits<1>(hs[il]));
}

double depth_sample(const void* src, int kind, int sW, int y, int x) {
  const int64_t px = (int64_t)y * sW + x;
  return kind == RR_DEPTH_U16 ? (double)rrresize::depth_metres(static_cast<const uint16_t*>(src)[px]) : (double)static_cast<const float*>(src)[px];
}

}  // namespace

extern "C" {

// one frame: src (sH x sW, `kind`) -> out H x W x 3 float64 B G R
int resize_emu_image(const void* src, int kind, int sH, int sW, int H, int W, double* out) {
  if (!src || !out || kind < RR_RESIZE_BGR_U8 || kind > RR_RESIZE_RGB_BF16 || sH <= 0 || sW <= 0 || H <= 0 || W <= 0) return RR_E_ARG;
  const bool identity = sH == H && sW == W;
  const double sx = rrresize::resize_scale(W, sW), sy = rrresize::resize_scale(H, sH);
  for (int y = 0; y < H; y++) {
    int32_t y0, y1;
    double wy;
    rrresize::resize_coord(y, sH, sy, y0, y1, wy);
    for (int x = 0; x < W; x++) {
      int32_t x0, x1;
      double wx;
      rrresize::resize_coord(x, sW, sx, x0, x1, wx);
      for (int c = 0; c < 3; c++)
        out[((int64_t)y * W + x) * 3 + c] =
            identity ? image_sample(src, kind, sH, sW, y0, x0, c)
                     : rrresize::resize_sample(image_sample(src, kind, sH, sW, y0, x0, c), image_sample(src, kind, sH, sW, y0, x1, c),
                                               image_sample(src, kind, sH, sW, y1, x0, c), image_sample(src, kind, sH, sW, y1, x1, c), wx, wy);
    }
  }
  return RR_OK;
}

// one frame: src (sH x sW uint16 samples or float32 metres) -> out H x W float32
int resize_emu_depth(const void* src, int kind, int sH, int sW, int H, int W, float* out) {
  if (!src || !out || (kind != 0 && kind != RR_DEPTH_U16) || sH <= 0 || sW <= 0 || H <= 0 || W <= 0) return RR_E_ARG;
  const bool identity = sH == H && sW == W;
  const double sx = rrresize::resize_scale(W, sW), sy = rrresize::resize_scale(H, sH);
  for (int y = 0; y < H; y++) {
    int32_t y0, y1;
    double wy;
    rrresize::resize_coord(y, sH, sy, y0, y1, wy);
    for (int x = 0; x < W; x++) {
      int32_t x0, x1;
      double wx;
      rrresize::resize_coord(x, sW, sx, x0, x1, wx);
      out[(int64_t)y * W + x] = identity ? (float)depth_sample(src, kind, sW, y0, x0)
                                         : (float)rrresize::resize_sample(depth_sample(src, kind, sW, y0, x0), depth_sample(src, kind, sW, y0, x1),
                                                                          depth_sample(src, kind, sW, y1, x0), depth_sample(src, kind, sW, y1, x1), wx, wy);
    }
  }
  return RR_OK;
}

}  // extern "C"
