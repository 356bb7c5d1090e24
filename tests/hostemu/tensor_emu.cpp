// tensor_emu.cpp -- the g++ build of csrc/rr_convert.h for the CPU tier (tests/test_tensor_formats_host.py): the conversions the
// ingest, finalize and resize kernels apply to float16 / bfloat16 elements, and the index of an interleaved frame's element,
// looped over arrays.  bf16: 0 = float16, 1 = bfloat16.
#include <stddef.h>
#include <stdint.h>

#include "rainhip.h"
#include "rr_convert.h"

extern "C" {

// n half patterns -> the bits of the float32 each widens to
int tensor_emu_widen(const uint16_t* in, int64_t n, int bf16, uint32_t* out) {
  if (!in || !out || n < 0 || (bf16 != 0 && bf16 != 1)) return RR_E_ARG;
  for (int64_t i = 0; i < n; i++) out[i] = bf16 ? rrconv::widen_bits<1>(in[i]) : rrconv::widen_bits<0>(in[i]);
  return RR_OK;
}

// n float32 patterns -> the half pattern each rounds to (nearest, ties to even)
int tensor_emu_narrow(const uint32_t* in, int64_t n, int bf16, uint16_t* out) {
  if (!in || !out || n < 0 || (bf16 != 0 && bf16 != 1)) return RR_E_ARG;
  for (int64_t i = 0; i < n; i++) out[i] = bf16 ? rrconv::narrow_bits<1>(in[i]) : rrconv::narrow_bits<0>(in[i]);
  return RR_OK;
}

// planar [n][3][npix] int32 -> interleaved [n][npix][3] through interleaved_index / planar_index
int tensor_emu_interleave(const int32_t* in, int64_t n, int64_t npix, int32_t* out) {
  if (!in || !out || n < 0 || npix < 0) return RR_E_ARG;
  for (int64_t f = 0; f < n; f++)
    for (int64_t p = 0; p < npix; p++)
      for (int c = 0; c < 3; c++)
        out[f * 3 * npix + rrconv::interleaved_index(p, c)] = in[f * 3 * npix + rrconv::planar_index(p, c, npix)];
  return RR_OK;
}

int tensor_emu_codes(int which) {
  switch (which) {
    case 0: return RR_TENSOR_F16;
    case 1: return RR_TENSOR_BF16;
    case 2: return RR_LAYOUT_PLANAR;
    case 3: return RR_LAYOUT_INTERLEAVED;
    case 4: return (int)sizeof(rr_tensor_batch);
    case 5: return (int)offsetof(rr_tensor_batch, layout);
    default: return -1;
  }
}

}  // extern "C"
