// rr_convert.h -- the element formats rr_augment_frames_device takes besides bytes and float32 (include/rainhip.h RR_TENSOR_F16 /
// RR_TENSOR_BF16, RR_LAYOUT_INTERLEAVED), stated once: the two half types <-> float32, and where an element of an
// interleaved frame lies.
//
// The RR_HD functions are called by the ingest, finalize and resize kernels of csrc/rr_tensor.h / rainhip.hip on gfx950 and by the
// g++ library of the CPU tier (tests/test_tensor_formats_host.py), which proves them equal, bit for bit, to torch's conversions on the CPU.
// Integer arithmetic on the bit patterns (one exact float multiplication for half subnormals): nothing a compiler flag or a
// denormal mode changes.
#pragma once
#include <stdint.h>
#include <string.h>

#if !defined(RR_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RR_HD __host__ __device__ inline
#else
#define RR_HD inline
#endif
#endif

namespace rrconv {

RR_HD uint32_t f32_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}
RR_HD float bits_f32(uint32_t u) {
  float v;
  memcpy(&v, &u, 4);
  return v;
}

// float16 / bfloat16 -> the float32 it widens to exactly; subnormals are values like any other, a NaN keeps its payload's top bits
RR_HD uint32_t half_to_f32_bits(uint16_t h) {
  const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 0) return s | f32_bits((float)m * 5.9604644775390625e-08f);      // m * 2^-24: exact, a normal float32 (or 0)
  if (e == 31) return s | 0x7f800000u | (m << 13);
  return s | ((e + 112u) << 23) | (m << 13);
}
RR_HD uint32_t bf16_to_f32_bits(uint16_t h) { return (uint32_t)h << 16; }

// float32 -> float16, round to nearest, ties to even: one rounding of the exact value (overflow to infinity from 65520 on)
RR_HD uint16_t f32_bits_to_half(uint32_t x) {
  const uint32_t s = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(s | 0x7e00u);                        // NaN
  if (a >= 0x477ff000u) return (uint16_t)(s | 0x7c00u);                       // >= 65520 (and infinity)
  if (a >= 0x38800000u) {                                                     // >= 2^-14: a normal half; a carry moves into the exponent
    uint32_t r = (a - (112u << 23)) >> 13;
    const uint32_t rem = a & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;
    return (uint16_t)(s | r);
  }
  const uint32_t e = a >> 23;
  if (e < 102u) return (uint16_t)s;                                           // < 2^-25: 0
  const uint32_t m = (a & 0x7fffffu) | 0x800000u, sh = 126u - e;              // the result counts units of 2^-24: m >> sh, sh in 14 .. 24
  uint32_t r = m >> sh;
  const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
  if (rem > half || (rem == half && (r & 1u))) r++;
  return (uint16_t)(s | r);
}
// float32 -> bfloat16, round to nearest, ties to even
RR_HD uint16_t f32_bits_to_bf16(uint32_t x) {
  if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)(((x >> 16) & 0x8000u) | 0x7fc0u);      // NaN: quiet, the sign kept as above
  return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
}

// BF16: 0 = float16, 1 = bfloat16 (a compile-time choice in the kernels)
template <int BF16>
RR_HD uint32_t widen_bits(uint16_t h) {
  return BF16 ? bf16_to_f32_bits(h) : half_to_f32_bits(h);
}
template <int BF16>
RR_HD uint16_t narrow_bits(uint32_t x) {
  return BF16 ? f32_bits_to_bf16(x) : f32_bits_to_half(x);
}

// an interleaved frame [H][W][3] RGB: the element index of channel c (0 = R) of pixel p = y W + x
RR_HD int64_t interleaved_index(int64_t p, int c) { return 3 * p + c; }
// ... and of a planar frame [3][H][W] of npix = H W pixels
RR_HD int64_t planar_index(int64_t p, int c, int64_t npix) { return (int64_t)c * npix + p; }

}  // namespace rrconv
