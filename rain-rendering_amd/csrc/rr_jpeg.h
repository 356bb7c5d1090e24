// rr_jpeg.h -- the parallel half of a baseline JPEG decoder, stated once.
// The host parses the file and decodes its Huffman stream (sequential by nature; rr_png.cpp) into a COEFFICIENT RECORD:
//   rr_jpeg_header | int16 coefficients, not dequantised, natural (de-zigzagged) order, 64 per block, the blocks of a
//   component in raster order over its plane padded to whole MCUs, Y then Cb then Cr.
// What is left is per block and per pixel -- dequantisation, the 8x8 inverse DCT, chroma upsampling, YCbCr -> B G R -- and
// runs on the device (k_jpeg_idct, k_jpeg_bgr in rainhip.hip), in rr_jpeg_read_bgr8 on the host and in the g++ test library through
// the functions below.  The arithmetic is libjpeg's (jidctint.c "islow", jdsample.c fancy upsampling, jdcolor.c) restated as
// two's-complement 32-bit arithmetic that WRAPS: every sum and product is formed on uint32_t, so device, host and the numpy
// statement of tests/jpeg_cases.py agree on every input, a damaged file's coefficients included.
#pragma once
#include <stdint.h>

#include "rainhip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RRJ_HD __host__ __device__ inline
#else
#define RRJ_HD inline
#endif

namespace rrjpeg {

// ---- the record's geometry ---------------------------------------------------------------------------------------------
struct Geom {
  int ncomp;                       // 1 (grey) or 3
  int hs, vs;                      // luma sampling factors = the MCU's size in blocks (chroma is always 1 x 1)
  int mw, mh;                      // MCUs across / down
  int pw[3], ph[3];                // the padded planes, in samples
  int dw, dh;                      // chroma's downsampled size ceil(W / hs) x ceil(H / vs): what upsampling reads
  int64_t blk0[3];                 // first block of a component in the record = its plane's offset / 64 in the plane block
  int64_t nblocks;                 // blocks of all components = plane bytes / 64
};
RRJ_HD bool geom_of(int W, int H, int sampling, Geom& g) {
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || sampling < RR_JPEG_444 || sampling > RR_JPEG_GREY) return false;
  g.ncomp = sampling == RR_JPEG_GREY ? 1 : 3;
  g.hs = (sampling == RR_JPEG_422 || sampling == RR_JPEG_420) ? 2 : 1;
  g.vs = sampling == RR_JPEG_420 ? 2 : 1;
  g.mw = (W + 8 * g.hs - 1) / (8 * g.hs);
  g.mh = (H + 8 * g.vs - 1) / (8 * g.vs);
  g.dw = (W + g.hs - 1) / g.hs;
  g.dh = (H + g.vs - 1) / g.vs;
  int64_t b = 0;
  for (int c = 0; c < 3; c++) {
    g.pw[c] = c < g.ncomp ? g.mw * 8 * (c ? 1 : g.hs) : 0;
    g.ph[c] = c < g.ncomp ? g.mh * 8 * (c ? 1 : g.vs) : 0;
    g.blk0[c] = b;
    b += (int64_t)(g.pw[c] / 8) * (g.ph[c] / 8);
  }
  g.nblocks = b;
  return true;
}
RRJ_HD int64_t record_bytes(const Geom& g) { return (int64_t)sizeof(rr_jpeg_header) + g.nblocks * 128; }

// ---- the inverse DCT (jidctint.c, CONST_BITS 13, PASS1_BITS 2) ---------------------------------------------------------
RRJ_HD int32_t sra(uint32_t v, int n) { return (int32_t)v >> n; }           // (arithmetic on every compiler this is built with)
// one 1-D pass: eight inputs -> the eight sums before descaling
RRJ_HD void idct_1d(const uint32_t i[8], uint32_t o[8]) {
  uint32_t z2 = i[2], z3 = i[6];
  uint32_t z1 = (z2 + z3) * 4433u;
  const uint32_t t2 = z1 - z3 * 15137u, t3 = z1 + z2 * 6270u;
  const uint32_t t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  z2 = a1 + a2;
  z3 = a0 + a2;
  uint32_t z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u;
  a1 *= 16819u;
  a2 *= 25172u;
  a3 *= 12299u;
  z1 = 0u - z1 * 7373u;
  z2 = 0u - z2 * 20995u;
  z3 = 0u - z3 * 16069u + z5;
  z4 = 0u - z4 * 3196u + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  o[0] = t10 + a3;
  o[1] = t11 + a2;
  o[2] = t12 + a1;
  o[3] = t13 + a0;
  o[4] = t13 - a0;
  o[5] = t12 - a1;
  o[6] = t11 - a2;
  o[7] = t10 - a3;
}
RRJ_HD uint32_t dequant(int16_t c, uint16_t q) { return (uint32_t)(int32_t)c * (uint32_t)q; }
RRJ_HD uint32_t idct_col_out(uint32_t v) { return (uint32_t)sra(v + (1u << 10), 11); }
RRJ_HD int idct_row_out(uint32_t v) {
  const int32_t s = sra(v + (1u << 17), 18) + 128;
  return s < 0 ? 0 : (s > 255 ? 255 : s);
}
// one block: 64 coefficients in natural order, the table in natural order -> 64 samples
RRJ_HD void jpeg_idct_islow(const int16_t* coef, const uint16_t* q, uint8_t* out) {
  uint32_t ws[64], in[8], o[8];
  for (int x = 0; x < 8; x++) {
    for (int y = 0; y < 8; y++) in[y] = dequant(coef[y * 8 + x], q[y * 8 + x]);
    idct_1d(in, o);
    for (int y = 0; y < 8; y++) ws[y * 8 + x] = idct_col_out(o[y]);
  }
  for (int y = 0; y < 8; y++) {
    idct_1d(ws + y * 8, o);
    for (int x = 0; x < 8; x++) out[y * 8 + x] = (uint8_t)idct_row_out(o[x]);
  }
}

// ---- chroma upsampling (jdsample.c) -------------------------------------------------------------------------------------
// One output sample each.  The "fancy" triangle filters run where the downsampled width dw exceeds 2; at dw <= 2 libjpeg
// replicates samples (its choice of method, jinit_upsampler), and so does this.
// row: a chroma row of dw samples; x: the output column, 0 <= x < 2 dw
RRJ_HD int jpeg_up_h2v1(const uint8_t* row, int dw, int x) {
  const int i = x >> 1;
  if (dw <= 2) return row[i];
  if (x & 1) return i == dw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
  return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
}
// pl: a chroma plane of dh rows of dw samples, `stride` samples apart; (x, y): the output sample, 0 <= x < 2 dw, 0 <= y < 2 dh
RRJ_HD int jpeg_up_h2v2(const uint8_t* pl, int64_t stride, int dw, int dh, int x, int y) {
  const int i = x >> 1, r = y >> 1;
  if (dw <= 2) return pl[r * stride + i];
  int r1 = (y & 1) ? r + 1 : r - 1;                     // the nearer neighbour row; outside the plane: the row itself
  r1 = r1 < 0 ? 0 : (r1 > dh - 1 ? dh - 1 : r1);
  const uint8_t *a = pl + r * stride, *b = pl + r1 * stride;
  const int s = 3 * a[i] + b[i];
  if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * a[i + 1] + b[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * a[i - 1] + b[i - 1] + 8) >> 4;
}

// ---- colour (jdcolor.c, SCALEBITS 16) -----------------------------------------------------------------------------------
RRJ_HD int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
RRJ_HD void jpeg_ycc_bgr(int y, int cb, int cr, uint8_t* bgr) {
  cb -= 128;
  cr -= 128;
  bgr[0] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
  bgr[1] = (uint8_t)clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  bgr[2] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
}

// One pixel of the frame from the component planes of bytes (at rr_jpeg planes' padded sizes): what k_jpeg_bgr and
// rr_jpeg_read_bgr8 do per pixel.
RRJ_HD void pixel_bgr(const uint8_t* planes, const Geom& g, int sampling, int x, int y, uint8_t* bgr) {
  const int Y = planes[(int64_t)y * g.pw[0] + x];
  if (sampling == RR_JPEG_GREY) {
    bgr[0] = bgr[1] = bgr[2] = (uint8_t)Y;
    return;
  }
  const uint8_t* pb = planes + g.blk0[1] * 64;
  const uint8_t* pr = planes + g.blk0[2] * 64;
  const int64_t cs = g.pw[1];
  int cb, cr;
  if (sampling == RR_JPEG_444) {
    cb = pb[y * cs + x];
    cr = pr[y * cs + x];
  } else if (sampling == RR_JPEG_422) {
    cb = jpeg_up_h2v1(pb + y * cs, g.dw, x);
    cr = jpeg_up_h2v1(pr + y * cs, g.dw, x);
  } else {
    cb = jpeg_up_h2v2(pb, cs, g.dw, g.dh, x, y);
    cr = jpeg_up_h2v2(pr, cs, g.dw, g.dh, x, y);
  }
  jpeg_ycc_bgr(Y, cb, cr, bgr);
}

}  // namespace rrjpeg
