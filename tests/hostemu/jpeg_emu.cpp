// jpeg_emu.cpp -- the g++ build of csrc/rr_jpeg.h (the arithmetic k_jpeg_idct / k_jpeg_bgr and rr_jpeg_read_bgr8 share) for
// tests/test_jpeg_host.py: every function on arrays, so that numpy can hold it against its own statement (tests/jpeg_cases.py).
#include <cstdint>

#include "rr_jpeg.h"

extern "C" {

// n blocks of 64 coefficients (natural order) through one table -> n blocks of 64 samples
void emu_jpeg_idct(const int16_t* coef, int64_t n, const uint16_t* q, uint8_t* out) {
  for (int64_t b = 0; b < n; b++) rrjpeg::jpeg_idct_islow(coef + b * 64, q, out + b * 64);
}
// dh rows of dw samples -> dh rows of 2 dw
void emu_jpeg_up_h2v1(const uint8_t* pl, int dh, int dw, uint8_t* out) {
  for (int y = 0; y < dh; y++)
    for (int x = 0; x < 2 * dw; x++) out[(int64_t)y * 2 * dw + x] = (uint8_t)rrjpeg::jpeg_up_h2v1(pl + (int64_t)y * dw, dw, x);
}
// dh rows of dw samples -> 2 dh rows of 2 dw
void emu_jpeg_up_h2v2(const uint8_t* pl, int dh, int dw, uint8_t* out) {
  for (int y = 0; y < 2 * dh; y++)
    for (int x = 0; x < 2 * dw; x++) out[(int64_t)y * 2 * dw + x] = (uint8_t)rrjpeg::jpeg_up_h2v2(pl, dw, dw, dh, x, y);
}
// n (Y, Cb, Cr) triples -> n (B, G, R) triples
void emu_jpeg_ycc_bgr(const uint8_t* ycc, int64_t n, uint8_t* bgr) {
  for (int64_t i = 0; i < n; i++) rrjpeg::jpeg_ycc_bgr(ycc[3 * i], ycc[3 * i + 1], ycc[3 * i + 2], bgr + 3 * i);
}
// a whole record (header + coefficients) -> the frame's B G R bytes, as k_jpeg_idct + k_jpeg_bgr make them; 0, or -1 for a bad header
int emu_jpeg_record_bgr(const uint8_t* rec, uint8_t* planes, uint8_t* bgr) {
  const rr_jpeg_header* h = reinterpret_cast<const rr_jpeg_header*>(rec);
  rrjpeg::Geom g;
  if (h->magic != RR_JPEG_MAGIC || !rrjpeg::geom_of(h->W, h->H, h->sampling, g)) return -1;
  const int16_t* coef = reinterpret_cast<const int16_t*>(h + 1);
  uint8_t blk[64];
  for (int c = 0; c < g.ncomp; c++) {
    const int bw = g.pw[c] / 8, bh = g.ph[c] / 8;
    for (int by = 0; by < bh; by++)
      for (int bx = 0; bx < bw; bx++) {
        rrjpeg::jpeg_idct_islow(coef + (g.blk0[c] + (int64_t)by * bw + bx) * 64, h->q[c], blk);
        for (int y = 0; y < 8; y++)
          for (int x = 0; x < 8; x++) planes[g.blk0[c] * 64 + ((int64_t)by * 8 + y) * g.pw[c] + bx * 8 + x] = blk[y * 8 + x];
      }
  }
  for (int y = 0; y < h->H; y++)
    for (int x = 0; x < h->W; x++) rrjpeg::pixel_bgr(planes, g, h->sampling, x, y, bgr + ((int64_t)y * h->W + x) * 3);
  return 0;
}
}
