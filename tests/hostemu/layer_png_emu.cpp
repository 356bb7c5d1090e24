// g++ build of the layer file's pixel (csrc/rr_layer.h layer_rgba) for tests/test_layer_png_host.py: the RR_HD statement
// k_rain_layer<2> calls on the device, compiled for the host with -ffp-contract=off, against tools/layer_png.py encode(); and the Sub
// filter of k_png_layer (a pixel minus its left neighbour, byte by byte, of two dwords) against sub_filter().
#include <cstdint>
#include <cstring>

#include "rainhip.h"
#include "rr_device.h"
#include "rr_lens.h"
#include "rr_layer.h"

extern "C" {

// n pixels of float32 (L_B, L_G, L_R, T) -> n pixels of bytes (R, G, B, A)
void rr_emu_layer_rgba(int64_t n, const float* layer, uint8_t* rgba) {
  for (int64_t i = 0; i < n; i++) {
    const uint32_t v = layer_rgba(layer[4 * i], layer[4 * i + 1], layer[4 * i + 2], layer[4 * i + 3]);
    memcpy(rgba + 4 * i, &v, 4);                          // (R in the low byte: the device's store, on a little-endian host)
  }
}

// [H][W][4] bytes -> H rows of 1 + 4 W bytes, filter type 1, with k_png_layer's word arithmetic
void rr_emu_layer_rows(int32_t H, int32_t W, const uint8_t* rgba, uint8_t* rows) {
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      uint32_t cur, left = 0u;
      memcpy(&cur, rgba + ((int64_t)y * W + x) * 4, 4);
      if (x > 0) memcpy(&left, rgba + ((int64_t)y * W + x - 1) * 4, 4);
      uint8_t* o = rows + (int64_t)y * (1 + 4 * W) + 1 + 4 * x;
      if (x == 0) o[-1] = 1;
      for (int c = 0; c < 4; c++) o[c] = (uint8_t)((cur >> (8 * c)) - (left >> (8 * c)));
    }
}

}  // extern "C"
