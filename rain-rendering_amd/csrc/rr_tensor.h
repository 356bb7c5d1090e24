// rr_tensor.h -- the kernels of rr_augment_frames_device (include/rainhip.h) that meet PyTorch's tensors:
//   k_planar_in<0> / k_planar_in<1>    [n][3][H][W] RGB (bytes, or float32 in [0, 1]) -> the interleaved BGR image the pre-pass and
//                                      the hot path read (RR_IN_BG_U8 / RR_IN_BG_F32): values moved, never converted
//   k_tensor_in<DT, IL>                the same for the six other formats: [n][H][W][3] bytes and float32 (IL), float16 and bfloat16
//                                      in either layout, widened into the float32 image (csrc/rr_convert.h)
//   k_finalize_planar                  in place of k_finalize16 / k_finalize: the frame's bytes (finalize_rgb) straight into the caller's
//                                      frame -- [3][H][W] planes or [H][W][3]; as bytes, as byte / 255 in float32, or as that float
//                                      rounded once to float16 / bfloat16 -- and float(mask_f64) into [H][W]
// Included by rainhip.hip inside its anonymous namespace, behind FrameDesc, Scratch and finalize_rgb.
#ifndef RR_TENSOR_H
#define RR_TENSOR_H

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

template <int Q>
__device__ inline u32x4_t funnel16(const uint32_t w[8], uint32_t r) {
  u32x4_t o;
  o.x = __builtin_amdgcn_alignbyte(w[Q + 1], w[Q], r);
  o.y = __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], r);
  o.z = __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], r);
  o.w = __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], r);
  return o;
}

// The 16 bytes at p, inside the buffer [lo, hi).  A plane of a [n][3][H][W] tensor starts wherever (c + 3 f) * H * W elements
// put it -- KITTI's H * W is 2 mod 4 -- but its misalignment p & 15 is the same for every lane of a wave (lanes step by 16 bytes):
// aligned planes take one dwordx4 load, the others the two aligned dwordx4 loads around the bytes and a funnel shift
// (v_alignbyte_b32), as long as both stay inside the buffer; the few windows at its very ends read byte by byte.
__device__ inline u32x4_t load16(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
  if (m == 0) return *as_global(reinterpret_cast<const u32x4_t*>(p));
  const uint8_t* al = p - m;
  if (al >= lo && al + 32 <= hi) {
    const global_ptr<const u32x4_t> s = as_global(reinterpret_cast<const u32x4_t*>(al));
    const u32x4_t a = s[0], b = s[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t r = m & 3u;
    switch (m >> 2) {
      case 0: return funnel16<0>(w, r);
      case 1: return funnel16<1>(w, r);
      case 2: return funnel16<2>(w, r);
      default: return funnel16<3>(w, r);
    }
  }
  const global_ptr<const uint8_t> s = as_global(p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 16; k++) w[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
  return u32x4_t{w[0], w[1], w[2], w[3]};
}

// bytes: 16 pixels per lane -- one 16-byte load per plane, three 16-byte stores of B G R triplets (the frame's scratch image starts
// on a 16-byte boundary and a lane's 48 bytes follow it).  The last pixels of a frame (H * W not a multiple of 16) byte by byte.
__device__ inline void planar_in_u8(const uint8_t* img, uint8_t* out, int64_t npix, int64_t out_stride, int64_t total) {
  const int f = blockIdx.y;
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (p0 >= npix) return;
  const uint8_t* rp = img + ((int64_t)f * 3 + 0) * npix + p0;
  const uint8_t* gp = img + ((int64_t)f * 3 + 1) * npix + p0;
  const uint8_t* bp = img + ((int64_t)f * 3 + 2) * npix + p0;
  const global_ptr<uint8_t> o = as_global(out + (int64_t)f * out_stride + p0 * 3);
  if (p0 + 16 <= npix) {
    const uint8_t* hi = img + total;
    const u32x4_t R = load16(rp, img, hi), G = load16(gp, img, hi), B = load16(bp, img, hi);
    const uint32_t pl[3][4] = {{B.x, B.y, B.z, B.w}, {G.x, G.y, G.z, G.w}, {R.x, R.y, R.z, R.w}};      // BGR order
    uint32_t ow[12];
#pragma unroll
    for (int k = 0; k < 12; k++) ow[k] = 0u;
#pragma unroll
    for (int p = 0; p < 16; p++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int k = 3 * p + c;
        ow[k >> 2] |= ((pl[c][p >> 2] >> (8 * (p & 3))) & 0xffu) << (8 * (k & 3));
      }
    const global_ptr<u32x4_t> o4 = reinterpret_cast<global_ptr<u32x4_t>>(o);
    o4[0] = u32x4_t{ow[0], ow[1], ow[2], ow[3]};
    o4[1] = u32x4_t{ow[4], ow[5], ow[6], ow[7]};
    o4[2] = u32x4_t{ow[8], ow[9], ow[10], ow[11]};
  } else {
    for (int64_t p = 0; p < npix - p0; p++) {
      o[3 * p + 0] = as_global(bp)[p];
      o[3 * p + 1] = as_global(gp)[p];
      o[3 * p + 2] = as_global(rp)[p];
    }
  }
}

// float32: 4 pixels per lane -- one 16-byte load per plane, three 16-byte stores
__device__ inline void planar_in_f32(const float* img, float* out, int64_t npix, int64_t out_stride, int64_t total) {
  const int f = blockIdx.y;
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= npix) return;
  const float* rp = img + ((int64_t)f * 3 + 0) * npix + p0;
  const float* gp = img + ((int64_t)f * 3 + 1) * npix + p0;
  const float* bp = img + ((int64_t)f * 3 + 2) * npix + p0;
  const global_ptr<float> o = as_global(out + (int64_t)f * out_stride + p0 * 3);
  if (p0 + 4 <= npix) {
    const uint8_t* lo = reinterpret_cast<const uint8_t*>(img);
    const uint8_t* hi = lo + total * 4;
    const u32x4_t R = load16(reinterpret_cast<const uint8_t*>(rp), lo, hi), G = load16(reinterpret_cast<const uint8_t*>(gp), lo, hi),
                  B = load16(reinterpret_cast<const uint8_t*>(bp), lo, hi);
    const global_ptr<u32x4_t> o4 = reinterpret_cast<global_ptr<u32x4_t>>(o);
    o4[0] = u32x4_t{B.x, G.x, R.x, B.y};
    o4[1] = u32x4_t{G.y, R.y, B.z, G.z};
    o4[2] = u32x4_t{R.z, B.w, G.w, R.w};
  } else {
    for (int64_t p = 0; p < npix - p0; p++) {
      o[3 * p + 0] = as_global(bp)[p];
      o[3 * p + 1] = as_global(gp)[p];
      o[3 * p + 2] = as_global(rp)[p];
    }
  }
}

// out_stride: elements between two frames of the interleaved scratch image; total: elements of the whole input batch
template <int F32>
__global__ __launch_bounds__(256) void k_planar_in(const void* img, void* out, int64_t npix, int64_t out_stride, int64_t total) {
  if (F32)
    planar_in_f32(static_cast<const float*>(img), static_cast<float*>(out), npix, out_stride, total);
  else
    planar_in_u8(static_cast<const uint8_t*>(img), static_cast<uint8_t*>(out), npix, out_stride, total);
}

// The six formats k_planar_in does not take.  One lane per 16-byte piece of a plane (16 / EL pixels), or per the 48 bytes that hold as
// many interleaved pixels: three load16 either way -- a frame starts 3 H W EL bytes behind the last one, so the misalignment is the
// same for every lane of a wave -- and 48 (bytes) or 96 (half types, widened) or 48 (float32) bytes of B G R out, as whole 16-byte
// stores (the frame's scratch image starts on a 16-byte boundary).  The last pixels of a frame element by element.
// out_stride, total: BYTES between two frames of the scratch image / of the whole input batch.
template <int DT, int IL>
__global__ __launch_bounds__(256) void k_tensor_in(const uint8_t* img, uint8_t* out, int64_t npix, int64_t out_stride, int64_t total) {
  static_assert(IL || DT == TF_F16 || DT == TF_BF16, "planar bytes and float32: k_planar_in");
  constexpr int EL = DT == TF_U8 ? 1 : (DT == TF_F32 ? 4 : 2), OEL = DT == TF_U8 ? 1 : 4;      // bytes per element in / in the scratch image
  constexpr int PX = 16 / EL, NW = PX * 3 * OEL / 4;                                         // a lane's pixels; the dwords it writes
  constexpr int BF = DT == TF_BF16;
  const int f = blockIdx.y;
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PX;
  if (p0 >= npix) return;
  const uint8_t* fb = img + (int64_t)f * 3 * npix * EL;
  uint8_t* o = out + (int64_t)f * out_stride + p0 * 3 * OEL;
  if (p0 + PX <= npix) {
    const uint8_t* hi = img + total;
    uint32_t w[12], ow[NW];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const u32x4_t v = load16(IL ? fb + rrconv::interleaved_index(p0, 0) * EL + 16 * k : fb + rrconv::planar_index(p0, k, npix) * EL, img, hi);
      w[4 * k + 0] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
    if constexpr (DT == TF_U8) {
      // R G B R | G B R G | B R G B -> B G R B | G R B G | R B G R, every 12 bytes: v_perm_b32 picks byte 0 .. 3 of its second
      // operand and 4 .. 7 of its first; the middle dword takes bytes of all three
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t a = w[3 * j], b = w[3 * j + 1], c = w[3 * j + 2];
        ow[3 * j + 0] = __builtin_amdgcn_perm(b, a, 0x05000102u);                                   // bytes 2 1 0 5
        ow[3 * j + 1] = __builtin_amdgcn_perm(c, __builtin_amdgcn_perm(b, a, 0x07000304u), 0x03040100u);      // 4 3 8 7
        ow[3 * j + 2] = __builtin_amdgcn_perm(c, b, 0x05060702u);                                   // 6 11 10 9
      }
    } else {
#pragma unroll
      for (int p = 0; p < PX; p++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const int e = IL ? (int)rrconv::interleaved_index(p, c) : c * PX + p;                     // the element among the lane's 48 bytes
          if constexpr (DT == TF_F32) ow[3 * p + 2 - c] = w[e];
          else ow[3 * p + 2 - c] = rrconv::widen_bits<BF>((uint16_t)(w[e >> 1] >> (16 * (e & 1))));
        }
    }
    const global_ptr<u32x4_t> o4 = reinterpret_cast<global_ptr<u32x4_t>>(as_global(o));
#pragma unroll
    for (int k = 0; k < NW / 4; k++) o4[k] = u32x4_t{ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]};
  } else {
    for (int64_t p = 0; p < npix - p0; p++)
      for (int c = 0; c < 3; c++) {
        const int64_t e = IL ? rrconv::interleaved_index(p0 + p, c) : rrconv::planar_index(p0 + p, c, npix);
        if constexpr (DT == TF_U8) as_global(o)[3 * p + 2 - c] = as_global(fb)[e];
        else if constexpr (DT == TF_F32) as_global(reinterpret_cast<uint32_t*>(o))[3 * p + 2 - c] = as_global(reinterpret_cast<const uint32_t*>(fb))[e];
        else as_global(reinterpret_cast<uint32_t*>(o))[3 * p + 2 - c] = rrconv::widen_bits<BF>(as_global(reinterpret_cast<const uint16_t*>(fb))[e]);
      }
  }
}

// four floats to p: one 16-byte store where p allows it, two 8-byte ones at 8 bytes, else one by one (cnt < 4: the frame's tail)
__device__ inline void store_f32x4(float* p, const float v[4], int cnt) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (cnt == 4 && (a & 15u) == 0) {
    *reinterpret_cast<global_ptr<u32x4_t>>(as_global(p)) =
        u32x4_t{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
  } else if (cnt == 4 && (a & 7u) == 0) {
    const global_ptr<u32x2_t> q = reinterpret_cast<global_ptr<u32x2_t>>(as_global(p));
    q[0] = u32x2_t{__float_as_uint(v[0]), __float_as_uint(v[1])};
    q[1] = u32x2_t{__float_as_uint(v[2]), __float_as_uint(v[3])};
  } else {
    for (int k = 0; k < cnt; k++) as_global(p)[k] = v[k];
  }
}

// four bytes (packed in w) to p: one 4-byte store, two 2-byte ones, or byte by byte
__device__ inline void store_u8x4(uint8_t* p, uint32_t w, int cnt) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (cnt == 4 && (a & 3u) == 0) {
    *reinterpret_cast<global_ptr<uint32_t>>(as_global(p)) = w;
  } else if (cnt == 4 && (a & 1u) == 0) {
    const global_ptr<uint16_t> q = reinterpret_cast<global_ptr<uint16_t>>(as_global(p));
    q[0] = (uint16_t)(w & 0xffffu);
    q[1] = (uint16_t)(w >> 16);
  } else {
    for (int k = 0; k < cnt; k++) as_global(p)[k] = (uint8_t)(w >> (8 * k));
  }
}

// N dwords holding a lane's elements of EL bytes, `bytes` of them to store, to p: whole stores of 16, 8 or 4 bytes where N, p and a
// full count allow -- a lane's run is 4 N bytes behind its neighbour's, so the choice is the same across a wave -- bytes also in
// pairs, else element by element (a frame's tail, or a frame that starts off a dword)
template <int N, int EL>
__device__ inline void store_packed(uint8_t* p, const uint32_t (&w)[N], int bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const bool full = bytes == 4 * N;
  if (N % 4 == 0 && full && (a & 15u) == 0) {
    const global_ptr<u32x4_t> q = reinterpret_cast<global_ptr<u32x4_t>>(as_global(p));
#pragma unroll
    for (int k = 0; k < N / 4; k++) q[k] = u32x4_t{w[4 * k], w[(4 * k + 1) % N], w[(4 * k + 2) % N], w[(4 * k + 3) % N]};
  } else if (N % 2 == 0 && full && (a & 7u) == 0) {
    const global_ptr<u32x2_t> q = reinterpret_cast<global_ptr<u32x2_t>>(as_global(p));
#pragma unroll
    for (int k = 0; k < N / 2; k++) q[k] = u32x2_t{w[2 * k], w[(2 * k + 1) % N]};
  } else if (full && (a & 3u) == 0) {
    const global_ptr<uint32_t> q = reinterpret_cast<global_ptr<uint32_t>>(as_global(p));
#pragma unroll
    for (int k = 0; k < N; k++) q[k] = w[k];
  } else if (EL == 1 && full && (a & 1u) == 0) {
    const global_ptr<uint16_t> q = reinterpret_cast<global_ptr<uint16_t>>(as_global(p));
#pragma unroll
    for (int k = 0; k < 2 * N; k++) q[k] = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
  } else {
#pragma unroll
    for (int e = 0; e < 4 * N / EL; e++)
      if (e * EL < bytes) {
        if (EL == 1) as_global(p)[e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
        else if (EL == 2) reinterpret_cast<global_ptr<uint16_t>>(as_global(p))[e] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
        else reinterpret_cast<global_ptr<uint32_t>>(as_global(p))[e] = w[e];
      }
  }
}

// k_finalize_planar's stores for the formats behind its two own: a thread's four pixels (cnt of them: the frame's tail) as interleaved
// elements -- 12 bytes, 48 (float32) or 24 (half types) per lane -- or as four halves, 8 bytes, per plane.  A float element is
// float(byte) / 255.0f, a half that float rounded once (rr_convert.h).
template <int DT, int IL>
__device__ inline void finalize_store(void* frame, int64_t pix0, int64_t npix, const uint32_t (&rgb)[4][3], int cnt) {
  constexpr int EL = DT == TF_U8 ? 1 : (DT == TF_F32 ? 4 : 2);
  auto bits = [&](int px, int ch) -> uint32_t {
    if constexpr (DT == TF_U8) {
      return rgb[px][ch];
    } else {
      const uint32_t v = __float_as_uint((float)((double)rgb[px][ch] / 255.0));      // = float(byte) / 255.0f, correctly rounded
      if constexpr (DT == TF_F32) return v;
      else return rrconv::narrow_bits<DT == TF_BF16>(v);
    }
  };
  uint8_t* base = static_cast<uint8_t*>(frame);
  if constexpr (IL) {
    constexpr int N = 3 * EL;
    uint32_t w[N];
#pragma unroll
    for (int k = 0; k < N; k++) w[k] = 0u;
#pragma unroll
    for (int px = 0; px < 4; px++)
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const int e = (int)rrconv::interleaved_index(px, ch) * EL;
        w[e >> 2] |= bits(px, ch) << (8 * (e & 3));
      }
    store_packed<N, EL>(base + rrconv::interleaved_index(pix0, 0) * EL, w, cnt * 3 * EL);
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const uint32_t w[2] = {bits(0, ch) | (bits(1, ch) << 16), bits(2, ch) | (bits(3, ch) << 16)};
      store_packed<2, EL>(base + rrconv::planar_index(pix0, ch, npix) * EL, w, cnt * EL);
    }
  }
}

// Four pixels per thread: the composite (any form, comp_load) -> finalize_rgb -> the three planes; float output is the byte / 255
// (what ToTensor makes of the PNG the driver writes).  The same pass turns the float64 mask into float32.
__global__ __launch_bounds__(256) void k_finalize_planar(const FrameDesc* frames, Dims dm, Scratch sc) {
  const int f = blockIdx.y;
  const int64_t npix = (int64_t)dm.H * dm.W;
  const int64_t pix0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (pix0 >= npix) return;
  const FrameDesc& fr = frames[f];
  const double diff = sc.means[f * 4 + 0] - sc.means[f * 4 + 1];
  const int cnt = (int)(npix - pix0 < 4 ? npix - pix0 : 4);
  uint32_t rgb[4][3];
  float mk[4] = {0.f, 0.f, 0.f, 0.f};
  const global_ptr<const double> m64 = as_global(fr.mask_f64) + pix0;
#pragma unroll
  for (int px = 0; px < 4; px++) {
    rgb[px][0] = rgb[px][1] = rgb[px][2] = 0u;
    if (px < cnt) {
      double c[3];
      comp_load(fr, pix0 + px, c);
      finalize_rgb(c, diff, rgb[px]);
      mk[px] = (float)m64[px];
    }
  }
  const int fmt = fr.planar_fmt;             // the same for a frame's every workgroup: a wave-uniform branch
  if (fmt == TF_F32) {
    float* base = static_cast<float*>(fr.planar) + pix0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      float v[4];
#pragma unroll
      for (int px = 0; px < 4; px++) v[px] = (float)((double)rgb[px][ch] / 255.0);      // = float(byte) / 255.0f, correctly rounded
      store_f32x4(base + ch * npix, v, cnt);
    }
  } else if (fmt == TF_U8) {
    uint8_t* base = static_cast<uint8_t*>(fr.planar) + pix0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
      store_u8x4(base + ch * npix, rgb[0][ch] | (rgb[1][ch] << 8) | (rgb[2][ch] << 16) | (rgb[3][ch] << 24), cnt);
  } else if (fmt == (TF_U8 | TF_INTERLEAVED)) {
    finalize_store<TF_U8, 1>(fr.planar, pix0, npix, rgb, cnt);
  } else if (fmt == (TF_F32 | TF_INTERLEAVED)) {
    finalize_store<TF_F32, 1>(fr.planar, pix0, npix, rgb, cnt);
  } else if (fmt == TF_F16) {
    finalize_store<TF_F16, 0>(fr.planar, pix0, npix, rgb, cnt);
  } else if (fmt == (TF_F16 | TF_INTERLEAVED)) {
    finalize_store<TF_F16, 1>(fr.planar, pix0, npix, rgb, cnt);
  } else if (fmt == TF_BF16) {
    finalize_store<TF_BF16, 0>(fr.planar, pix0, npix, rgb, cnt);
  } else {
    finalize_store<TF_BF16, 1>(fr.planar, pix0, npix, rgb, cnt);
  }
  store_f32x4(fr.mask_f32 + pix0, mk, cnt);
}

#endif  // RR_TENSOR_H
