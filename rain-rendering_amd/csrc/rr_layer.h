// rr_layer.h -- the rain layer of a frame (include/rainhip.h rr_pipeline_set_layer / rr_augment_set_layer): what the
// streaks add to a pixel and how much of the background survives under them, without the background.
//   k_rain_layer<PLANAR>   walks the compositor's own lists and leaves (L_B, L_G, L_R, T) per pixel: one 16-byte store into
//                          [H][W][4], or (PLANAR) four 4-byte stores into the planes R, G, B, T of [4][H][W]
//   k_layer_finish         behind k_means: the frame's mean shift (the diff every finalize kernel subtracts) as one double, and
//                          the fogged background the compositor read as planar float32 RGB (rr_tensor_layer.background_out)
// Both are launched only when a layer is armed; neither compositor, none of their inputs and no launch of an unarmed call changes.
//
// The contract.  For pixel p of frame f take the drops the compositor lists for p, in table order.  A is the drop's alpha sample
// at p (a float64 of the arena), 0 outside the drop's footprint and, under RR_OPT_DEPTH_OCCLUSION, 0 where the drop is behind the
// scene (k_composite32's rule: hidden where zdist > scene depth).  Start with T = 1, L = (0, 0, 0); per drop
//     u = 1 - A te;   L_c <- u L_c + A kg_c  (c = B, G, R);   T <- u T
// with te = tau_one / exposure and kg_c = K_c g, the drop's blend factors exactly as k_colour leaves them in CompRec32.  There is
// no clamp anywhere.  The device carries T and L in float32, one IEEE operation per step, no contraction:
//     Af = float(A);  u = fma(Af, -te, 1);  L_c = fma(u, L_c, Af * kg_c);  T = u * T
// An entry flagged slow (CompRec32.pitch_slow bit 31: a factor that is not tame, or a caller's tile) takes the float64 factors
// of CompRec instead -- te = tau_one / exposure, kg_c = K_c g, not rounded to float -- and makes the step in float64 on
// double(L_c), double(T): u = 1 - A te, L_c = float(u L_c + A kg_c), T = float(u T): one rounding per value and step.
// A pixel no listed drop reaches keeps T == 1 and L == 0 exactly (alpha 0 gives u == 1: fma(1, L, 0) == L).
//
// Wherever no blend of the compositor clamped, its composite is T rainy_bg + L (the compositor's own float chain rounds
// differently: 1e-4 at the worst, one code of the uint8 image), so with shift = means[4 f] - means[4 f + 1]
//     rainy_rgb = uint8(clip01(T rainy_bg + L - shift) 255)          within 1 LSB
// Sufficient for "no blend clamped": the inputs lie in [0, 1] and kg_c <= te for every listed drop -- each blend is then a convex
// combination of the pixel and kg_c / te.  The layer knows nothing of the lens pass, exactly like the mask.
//
// The layer FILE (rr_pipeline_set_layer_png): the pixel as straight-alpha 8-bit RGBA, layer_rgba() below -- the
// RR_HD statement k_rain_layer<2> calls on gfx950 and g++ compiles for the CPU tier (tests/test_layer_png_host.py), which holds it
// equal, byte for byte, to its numpy statement in rain-rendering_amd/tools/layer_png.py (encode).
//   k_rain_layer<2>        the same walk with the byte store: 4 bytes per pixel into the slot's [n][H][W][4] RGBA staging, and the
//                          16-byte float pixel as well where the frame's float layer is armed
//   k_png_layer            the staging as the file's scanlines: H rows of 1 + 4 W bytes, filter type 1 (Sub)
//
// Included by rainhip.hip inside its anonymous namespace, behind k_composite32 (TILE32_H, float2_t, u32x4_t), FrameDesc and Scratch;
// the statement alone by a g++ source, behind rr_device.h and rr_lens.h.
#ifndef RR_LAYER_H
#define RR_LAYER_H

// One pixel of the layer file from its float32 (L_B, L_G, L_R, T): the bytes R, G, B, A of a straight-alpha RGBA pixel, R in the
// low byte of the word.  a = 1 - T in float32; A8 = clamp(rint(a * 255.0f), 0, 255), half to even, NaN -> 0 (lens_round_u8's rule);
// the colour is divided by the QUANTISED alpha, in double: C_c = clamp(rint(L_c * (65025 / A8)), 0, 255), NaN -> 0; A8 == 0 gives
// (0, 0, 0, 0).  The reader's T' = 1 - A8 / 255, L'_c = A8 C_c / 65025 then recompose over x as T' x + L' (PNG's `over`).
RR_HD uint8_t layer_colour_u8(float l, double q) { return (uint8_t)(int)fmin(fmax(rint((double)l * q), 0.0), 255.0); }
RR_HD uint32_t layer_rgba(float lb, float lg, float lr, float T) {
  const float a = 1.0f - T;
  const uint32_t A8 = rrlens::lens_round_u8(a * 255.0f);
  if (A8 == 0u) return 0u;
  const double q = 65025.0 / (double)A8;
  return (uint32_t)layer_colour_u8(lr, q) | ((uint32_t)layer_colour_u8(lg, q) << 8) | ((uint32_t)layer_colour_u8(lb, q) << 16) | (A8 << 24);
}

#if defined(__HIPCC__)

// where one frame's layer goes (device pointers, each may be null); uploaded per batch beside the frame descriptors
struct LayerDesc {
  float* layer;                      // [H][W][4] (L_B, L_G, L_R, T), 16-byte aligned; planar: [4][H][W] in the order R, G, B, T
  double* shift;                     // one double
  float* background;                 // [3][H][W] R, G, B: float(rainy_bg), the values the compositor read
  int32_t planar, want_rgba;         // want_rgba (k_rain_layer<2>, k_png_layer): the frame's layer file is asked for
};
static_assert(sizeof(LayerDesc) == 32, "LayerDesc is uploaded as 4-byte words");

typedef float float4_t __attribute__((ext_vector_type(4)));

// MODE 2's own argument, the pack Extra of k_rain_layer<2, LayerBytes>: the slot's RGBA staging, frame f at rgba + f * stride (a
// multiple of 4).  MODE 0 and 1 are instantiated with an empty pack: their arguments are what they were.
struct LayerBytes {
  uint8_t* rgba;
  int64_t stride;
};
template <class T>
__device__ inline const T& layer_extra(const T& t) { return t; }

// The walk is k_composite32's: the same coarse list, the same split into four wave quadrants of a 16 x 32 tile, the same entry
// order, a lane's two pixels eight rows apart -- so the layer sees exactly the entries the image saw.  What made that loop fast is
// kept: the records of up to 64 entries in twelve vector registers handed out by v_readlane, the samples requested two entries
// ahead behind static load counts, a sample outside the footprint read from the frame's zero line.  It loads no image, builds no
// mask and reduces nothing over the tile.
// MODE: 0 the interleaved float pixel, 1 (PLANAR) the four float planes, 2 the file's RGBA bytes -- quantised in registers
// (layer_rgba), one 4-byte store per pixel, a wave row of eight lanes 32 contiguous bytes -- and the interleaved float pixel too
// where the frame has a float layer: the one walk stores both.
template <int MODE, class... Extra>
__global__ __launch_bounds__(256) void k_rain_layer(const FrameDesc* frames, const LayerDesc* outs, Dims dm, double exposure, int max_drops,
                                                    int tiles_x, int tiles_y, int ctiles_x, int nct, int64_t arena_cap, Scratch sc, Extra... extra) {
  static_assert(sizeof...(Extra) == (MODE == 2 ? 1 : 0), "MODE 2 takes LayerBytes, MODE 0 and 1 nothing");
  constexpr int PLANAR = MODE == 1;
  const int f = blockIdx.y;
  const int ntiles = tiles_x * tiles_y, per_xcd = (ntiles + 7) / 8;
  const int tile = (int)(blockIdx.x % 8) * per_xcd + (int)(blockIdx.x / 8);      // XCD k: the k-th eighth of the tiles (shared L2)
  if (tile >= ntiles) return;
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // the descriptors' fields once, as scalar loads through the constant address space, before the first store (see k_composite32)
  const const_ptr<FrameDesc> fr = as_constant(frames + f);
  const const_ptr<LayerDesc> od = as_constant(outs + f);
  const void* const fr_depth = fr->depth;
  const int fr_depth_f64 = fr->depth_f64;
  float* const out = od->layer;
  bool want_rgba = false;
  if constexpr (MODE == 2) want_rgba = od->want_rgba != 0;
  if (!out && !want_rgba) return;                                   // (the frame asks for its shift alone)
  const int tx0 = txi * TILE, ty0 = tyi * TILE32_H, tx1 = min(tx0 + TILE, dm.W), ty1 = min(ty0 + TILE32_H, dm.H);
  const int px = tx0 + 8 * (wave & 1) + (lane & 7);
  const int py0 = ty0 + 16 * (wave >> 1) + (lane >> 3), py1 = py0 + 8;
  const bool live0 = px < dm.W && py0 < dm.H, live1 = px < dm.W && py1 < dm.H;
  const int64_t pix0 = (int64_t)py0 * dm.W + px, pix1 = (int64_t)py1 * dm.W + px;
  const int ct = (ty0 / CTILE) * ctiles_x + (tx0 / CTILE);
  const uint16_t* clist = sc.clist + ((int64_t)f * nct + ct) * max_drops;
  const int4* bbox = sc.bbox + (int64_t)f * max_drops;
  const int i_first = imin((int)as_global(clist)[imin(t, max_drops - 1)], max_drops - 1);      // (past the list's end: any valid index)
  const int4 bb_first = bbox[i_first];
  double scene0 = 1.0e300, scene1 = 1.0e300;
  if (fr_depth) {                    // (a pixel outside the frame reads the tile's first pixel: no lane branches around a load)
    const int64_t pq = (int64_t)ty0 * dm.W + tx0, pq0 = live0 ? pix0 : pq, pq1 = live1 ? pix1 : pq;
    if (fr_depth_f64) {
      scene0 = as_global((const double*)fr_depth)[pq0];
      scene1 = as_global((const double*)fr_depth)[pq1];
    } else {
      const float d0 = as_global((const float*)fr_depth)[pq0], d1 = as_global((const float*)fr_depth)[pq1];
      scene0 = (double)d0;
      scene1 = (double)d1;
    }
    scene0 = live0 ? scene0 : 1.0e300;
    scene1 = live1 ? scene1 : 1.0e300;
  }
  const bool has_depth = fr_depth != nullptr;
  float2_t l0 = {0.f, 0.f}, l1 = {0.f, 0.f}, l2 = {0.f, 0.f}, tr = {1.f, 1.f};      // L_B, L_G, L_R, T of (pixel 0, pixel 1)
  const CompRec32* comp = sc.comp32 + (int64_t)f * max_drops;
  const CompRec* comp64 = sc.comp + (int64_t)f * max_drops;
  const double* arena = sc.arena;
  const int n = sc.ccount[(int64_t)f * nct + ct];
  __shared__ int s_list[4][256];
  __shared__ int s_cnt[4][4];
  const int xm = tx0 + 8, ym = ty0 + 16;
  const float2_t one2 = {1.f, 1.f};
  const int64_t zero_at = (int64_t)f * arena_cap;                  // the frame's all-zero arena line (k_scan)
  for (int base = 0; base < n; base += 256) {
    const int k = base + t;
    unsigned hitm = 0;
    int i = 0;
    if (k < n) {
      i = base == 0 ? i_first : (int)clist[k];
      const int4 bb = base == 0 ? bb_first : bbox[i];
      if (bb.x < tx1 && bb.z > tx0 && bb.y < ty1 && bb.w > ty0) {
        const unsigned xl = bb.x < xm, xr = bb.z > xm, yt = bb.y < ym, yb = bb.w > ym;
        hitm = (xl & yt) | ((xr & yt) << 1) | ((xl & yb) << 2) | ((xr & yb) << 3);
      }
    }
    unsigned long long bal[4];
#pragma unroll
    for (int q = 0; q < 4; q++) bal[q] = __ballot((hitm >> q) & 1u);
    if (lane < 4) s_cnt[wave][lane] = __popcll(lane == 0 ? bal[0] : (lane == 1 ? bal[1] : (lane == 2 ? bal[2] : bal[3])));
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      int off = 0, tq = 0;
      for (int w = 0; w < 4; w++) {
        const int cw = s_cnt[w][q];
        if (w < wave) off += cw;
        tq += cw;
      }
      if ((hitm >> q) & 1u) s_list[q][off + __popcll(bal[q] & ((1ull << lane) - 1ull))] = i;
      if (q == wave) total = tq;
    }
    __syncthreads();
    const int* lst = s_list[wave];
    total = __builtin_amdgcn_readfirstlane(total);
    for (int sub = 0; sub < total; sub += 64) {
      const int nb = imin(64, total - sub);
      const int my = lst[sub + imin(lane, nb - 1)];               // this lane's entry: its drop
      const auto rp = as_global(reinterpret_cast<const u32x4_t*>(comp + my));
      const u32x4_t ra = rp[0], rb = rp[1], rc = rp[2];
      auto rl = [](uint32_t v, int j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, j); };
      // the two samples of entry j (a pixel outside the footprint, and every pixel of an entry past the batch, reads the
      // frame's zero line: the sample IS 0.0)
      auto issue = [&](int j, double& An0, double& An1) {
        const int jj = imin(j, nb - 1);
        const uint32_t xx = rl(ra.x, jj), yy = rl(ra.y, jj);
        const int64_t bs = (int64_t)(((uint64_t)rl(ra.w, jj) << 32) | (uint64_t)rl(ra.z, jj));
        const int pitch = (int)(rl(rb.x, jj) & 0x7fffffffu);
        const int x0 = (int)(xx & 0xffffu), x1 = (int)(xx >> 16), y0 = (int)(yy & 0xffffu), y1 = (int)(yy >> 16);
        const bool inx = (px >= x0) & (px < x1) & (j < nb);
        const bool in0 = inx & live0 & (py0 >= y0) & (py0 < y1), in1 = inx & live1 & (py1 >= y0) & (py1 < y1);
        const int64_t o0 = in0 ? bs + ((int64_t)py0 * pitch + px) : zero_at;
        const int64_t o1 = in1 ? bs + ((int64_t)py1 * pitch + px) : zero_at;
        An0 = arena[o0];
        An1 = arena[o1];
      };
      auto step = [&](int j, double Acur0, double Acur1) {
        double A0 = Acur0, A1 = Acur1;                            // (0.0 outside the footprint)
        if (has_depth) {                                          // depth-occlusion option: hidden where the drop is behind the scene
          const double z = __hiloint2double((int)rl(rc.w, j), (int)rl(rc.z, j));
          A0 = (z > scene0) ? 0.0 : Acur0;
          A1 = (z > scene1) ? 0.0 : Acur1;
        }
        if ((rl(rb.x, j) >> 31) != 0u) {                          // (wave-uniform) a slow entry: the float64 factors of CompRec
          const const_ptr<CompRec> r64 = as_constant(comp64) + __builtin_amdgcn_readlane(my, j);
          const double te = r64->tau_one / exposure, g = r64->g;
          const double k0 = r64->K[0] * g, k1 = r64->K[1] * g, k2 = r64->K[2] * g;
          const double u0 = 1.0 - A0 * te, u1 = 1.0 - A1 * te;
          l0 = float2_t{(float)(u0 * (double)l0.x + A0 * k0), (float)(u1 * (double)l0.y + A1 * k0)};
          l1 = float2_t{(float)(u0 * (double)l1.x + A0 * k1), (float)(u1 * (double)l1.y + A1 * k1)};
          l2 = float2_t{(float)(u0 * (double)l2.x + A0 * k2), (float)(u1 * (double)l2.y + A1 * k2)};
          tr = float2_t{(float)(u0 * (double)tr.x), (float)(u1 * (double)tr.y)};
        } else {
          const float te = __uint_as_float(rl(rb.y, j)), k0 = __uint_as_float(rl(rb.z, j)), k1 = __uint_as_float(rl(rb.w, j)),
                      k2 = __uint_as_float(rl(rc.x, j));
          const float2_t Af = {(float)A0, (float)A1};
          const float2_t u = __builtin_elementwise_fma(Af, float2_t{-te, -te}, one2);        // 1 - A te
          l0 = __builtin_elementwise_fma(u, l0, Af * k0);         // (1 - A te) L + A kg: no clamp
          l1 = __builtin_elementwise_fma(u, l1, Af * k1);
          l2 = __builtin_elementwise_fma(u, l2, Af * k2);
          tr = u * tr;
        }
      };
      double A00, A01, A10, A11, A20, A21;
      issue(0, A00, A01);
      issue(1, A10, A11);
      // whole triples in a loop without an early exit, the last one or two entries behind it; every step issues exactly two
      // loads, so the counts are static (see k_composite32)
      int e = 0;
      for (; e + 3 <= nb; e += 3) {
        issue(e + 2, A20, A21);
        step(e, A00, A01);
        issue(e + 3, A00, A01);
        step(e + 1, A10, A11);
        issue(e + 4, A10, A11);
        step(e + 2, A20, A21);
      }
      if (e < nb) step(e, A00, A01);
      if (e + 1 < nb) step(e + 1, A10, A11);
      // the (zero-line) samples requested past the batch's end are waited for here (see k_composite32)
      asm volatile("" ::"v"(A00), "v"(A01), "v"(A10), "v"(A11));
    }
    __syncthreads();
  }
  if (PLANAR) {                      // planes R, G, B, T: four stores per pixel, a wave row of eight lanes 32 contiguous bytes per plane
    const int64_t np = (int64_t)dm.H * dm.W;
    const global_ptr<float> o = as_global(out);
    if (live0) { o[pix0] = l2.x; o[np + pix0] = l1.x; o[2 * np + pix0] = l0.x; o[3 * np + pix0] = tr.x; }
    if (live1) { o[pix1] = l2.y; o[np + pix1] = l1.y; o[2 * np + pix1] = l0.y; o[3 * np + pix1] = tr.y; }
  } else if constexpr (MODE == 2) {   // (both pointers wave-uniform: scalar loads of the descriptor)
    if (want_rgba) {
      const LayerBytes& bytes = layer_extra(extra...);
      const global_ptr<uint32_t> o = as_global(reinterpret_cast<uint32_t*>(bytes.rgba + (int64_t)f * bytes.stride));
      if (live0) o[pix0] = layer_rgba(l0.x, l1.x, l2.x, tr.x);
      if (live1) o[pix1] = layer_rgba(l0.y, l1.y, l2.y, tr.y);
    }
    if (out) {
      const global_ptr<float4_t> o = as_global(reinterpret_cast<float4_t*>(out));
      if (live0) o[pix0] = float4_t{l0.x, l1.x, l2.x, tr.x};
      if (live1) o[pix1] = float4_t{l0.y, l1.y, l2.y, tr.y};
    }
  } else {
    const global_ptr<float4_t> o = as_global(reinterpret_cast<float4_t*>(out));
    if (live0) o[pix0] = float4_t{l0.x, l1.x, l2.x, tr.x};
    if (live1) o[pix1] = float4_t{l0.y, l1.y, l2.y, tr.y};
  }
}

// The layer file of a frame, ready for deflate: what k_png_image makes of an image, of the RGBA staging k_rain_layer<2> left -- H rows
// of 1 + 4 W bytes, filter type 1 (Sub).  A pixel and its left neighbour are two aligned dwords of the staging; the row's bytes start
// at an odd address, so they leave as bytes.  A frame whose file is not asked for is left alone.
__global__ __launch_bounds__(256) void k_png_layer(const LayerDesc* outs, const uint8_t* rgba, int64_t rgba_stride, uint8_t* rows, int64_t rows_stride,
                                                   Dims dm) {
  const int f = blockIdx.y;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!as_constant(outs + f)->want_rgba || pix >= (int64_t)dm.H * dm.W) return;
  const int y = (int)(pix / dm.W), x = (int)(pix - (int64_t)y * dm.W);
  const global_ptr<const uint32_t> s = as_global(reinterpret_cast<const uint32_t*>(rgba + (int64_t)f * rgba_stride)) + pix;
  const uint32_t cur = s[0], left = x > 0 ? s[-1] : 0u;
  const global_ptr<uint8_t> o = as_global(rows) + (int64_t)f * rows_stride + (int64_t)y * (1 + 4 * dm.W) + 1 + 4 * x;
  if (x == 0) o[-1] = 1;                                // filter type: Sub
#pragma unroll
  for (int c = 0; c < 4; c++) o[c] = (uint8_t)((cur >> (8 * c)) - (left >> (8 * c)));
}

// Behind k_means: the frame's mean shift, and (rr_tensor_layer.background_out) the image the compositor blended over -- rainy_bg,
// whatever its element type -- as planar float32 R G B.  The float32 fog layer of rr_augment_frames_device leaves bit for bit.
__global__ __launch_bounds__(256) void k_layer_finish(const FrameDesc* frames, const LayerDesc* outs, Dims dm, Scratch sc) {
  const int f = blockIdx.y;
  const LayerDesc& od = outs[f];
  if (blockIdx.x == 0 && threadIdx.x == 0 && od.shift) *as_global(od.shift) = sc.means[f * 4 + 0] - sc.means[f * 4 + 1];
  if (!od.background) return;
  const int64_t npix = (int64_t)dm.H * dm.W, pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const FrameDesc& fr = frames[f];
  double in[3];
  load_px3(fr.rainy_bg, rainy_kind(fr), pix, in);
  const global_ptr<float> o = as_global(od.background) + pix;
  o[0] = (float)in[2];                                              // B G R -> R G B
  o[npix] = (float)in[1];
  o[2 * npix] = (float)in[0];
}

#endif  // __HIPCC__

#endif  // RR_LAYER_H
