// rr_jpeg_read.h -- the sequential half of the baseline JPEG decoder (host only; included by rr_png.cpp): the marker parser and the
// Huffman decoder that turn a file into its coefficient record (include/rainhip.h, csrc/rr_jpeg.h).  ITU-T T.81: SOI, APPn, COM,
// DQT (8-bit tables), SOF0, DHT, DRI, SOS, RSTn, EOI; byte un-stuffing; restart intervals.  Everything else is refused with a
// status and a one-line reason -- nothing here trusts a length, a table index or a code it has not checked.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "rr_jpeg.h"

namespace rrjpeg {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Refusal {                   // a status and its reason (the reason: a literal, or text formatted into buf)
  char buf[160];
  int fail(int code, const char* why) {
    snprintf(buf, sizeof buf, "%s", why);
    return code;
  }
};

struct HuffTable {
  bool defined = false;
  uint8_t vals[256];
  int32_t maxcode[18];             // largest code of length l (-1: none), [17] a sentinel
  int32_t valoff[17];              // index of the first value of length l less its first code
  uint16_t fast[512];              // 9 leading bits -> (length << 8) | value, 0 where the code is longer
  int32_t fast_ac[512];            // (as an AC table) 9 leading bits -> (coefficient << 8) | (run << 4) | bits used, where code and
                                   // magnitude bits fit the 9 together; 0 elsewhere
  // BITS / HUFFVAL (T.81 annex C): false where the counts describe no prefix code -- decided for a length BEFORE any of its codes
  // is entered (an over-subscribed length would index past the look-up table)
  bool build(const uint8_t* counts, const uint8_t* v, int nv) {
    defined = false;
    memcpy(vals, v, (size_t)nv);
    memset(fast, 0, sizeof fast);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
      valoff[l] = k - code;
      if (code + (int32_t)counts[l - 1] > (1 << l)) return false;
      for (int i = 0; i < counts[l - 1]; i++, k++, code++) {
        if (l <= 9) {
          const int lo = code << (9 - l);
          for (int j = 0; j < (1 << (9 - l)); j++) fast[lo + j] = (uint16_t)((l << 8) | vals[k]);
        }
      }
      maxcode[l] = counts[l - 1] ? code - 1 : -1;
      code <<= 1;
    }
    maxcode[17] = 0x7fffffff;
    for (int i = 0; i < 512; i++) {
      fast_ac[i] = 0;
      const int len = fast[i] >> 8, run = (fast[i] >> 4) & 15, sz = fast[i] & 15;
      if (len && sz && len + sz <= 9) {
        const int32_t v = (i >> (9 - len - sz)) & ((1 << sz) - 1);
        const int32_t c = v >= (1 << (sz - 1)) ? v : v - (1 << sz) + 1;
        fast_ac[i] = c * 256 + (run << 4) + (len + sz);
      }
    }
    defined = true;
    return true;
  }
};

// MSB-first bits of the entropy-coded segment: FF 00 is the byte FF; any other FF xx is a marker, where the reader stops and
// supplies zero bits, counting them -- a decoder that has used one of those has run out of data.
struct BitReader {
  const uint8_t *p, *end;
  uint64_t acc = 0;
  int n = 0;                       // valid bits in acc (its low n bits)
  int pad = 0;                     // zero bits supplied past the data
  void fill() {
    if (n > 32) return;
    if (p + 4 <= end) {                                 // four bytes at once where none of them is FF
      const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
      const uint32_t v = ~w;
      if (!((v - 0x01010101u) & ~v & 0x80808080u)) {
        acc = (acc << 32) | w;
        n += 32;
        p += 4;
        return;
      }
    }
    while (n <= 56) {
      uint32_t b = 0;
      if (p < end && (p[0] != 0xFF || (p + 1 < end && p[1] == 0x00))) {
        b = p[0];
        p += b == 0xFF ? 2 : 1;
      } else {
        pad += 8;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  uint32_t peek(int k) { return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1); }   // 1 <= k <= 16, after fill()
  void skip(int k) { n -= k; }
  bool overrun() const { return pad > n; }                                          // a supplied bit has been consumed
  void restart() {                                                                  // byte-align: drop what is buffered
    acc = 0;
    n = 0;
    pad = 0;
  }
};

inline int decode_symbol(BitReader& br, const HuffTable& t) {                       // -1: a code that is not in the table
  br.fill();
  const uint16_t f = t.fast[br.peek(9)];
  if (f) {
    br.skip(f >> 8);
    return f & 255;
  }
  int32_t code = (int32_t)br.peek(10);
  int l = 10;
  while (l <= 16 && code > t.maxcode[l]) {
    l++;
    if (l <= 16) code = (int32_t)br.peek(l);
  }
  if (l > 16) return -1;
  br.skip(l);
  return t.vals[(code + t.valoff[l]) & 255];
}
inline int32_t receive_extend(BitReader& br, int s) {                               // T.81 F.2.2.1; 0 <= s <= 15
  if (!s) return 0;
  br.fill();
  const int32_t v = (int32_t)br.peek(s);
  br.skip(s);
  return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
}

struct Frame {
  int32_t W = 0, H = 0, ncomp = 0, sampling = -1;
  int32_t want_W = 0, want_H = 0;  // set by the caller: the size the file must have (0: any), checked before the scan is decoded
  uint8_t id[3], tq[3], td[3], ta[3];
};

// A file's bytes -> its frame description and, where coef is given, its coefficient record's body (hdr filled likewise).
// coef has room for cap_blocks blocks.  RR_OK, or a refusal with its reason in r.
inline int read_jpeg(const uint8_t* b, size_t size, Frame& fr, rr_jpeg_header* hdr, int16_t* coef, int64_t cap_blocks, Refusal& r) {
  uint16_t qt[4][64];
  bool have_q[4] = {false, false, false, false}, have_sof = false;
  static thread_local HuffTable ht[2][4];
  for (int c = 0; c < 2; c++)
    for (int i = 0; i < 4; i++) ht[c][i].defined = false;
  int32_t dri = 0;
  if (size < 4 || b[0] != 0xFF || b[1] != 0xD8) return r.fail(RR_E_PARSE, "jpeg: no SOI marker");
  size_t p = 2;
  for (;;) {
    if (p + 2 > size) return r.fail(RR_E_PARSE, "jpeg: the file ends before its scan");
    if (b[p] != 0xFF) return r.fail(RR_E_PARSE, "jpeg: a marker was expected");
    while (p < size && b[p] == 0xFF) p++;                                         // (fill bytes)
    if (p >= size) return r.fail(RR_E_PARSE, "jpeg: the file ends before its scan");
    const int m = b[p++];
    if (m == 0xD8 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return r.fail(RR_E_PARSE, "jpeg: a marker out of place");
    if (m == 0xD9) return r.fail(RR_E_PARSE, "jpeg: EOI before any scan");
    if (p + 2 > size) return r.fail(RR_E_PARSE, "jpeg: a segment is cut short");
    const size_t L = ((size_t)b[p] << 8) | b[p + 1];
    if (L < 2 || p + L > size) return r.fail(RR_E_PARSE, "jpeg: a segment is cut short");
    const uint8_t* seg = b + p + 2;
    const size_t n = L - 2;
    p += L;
    if (m == 0xDB) {                                                              // DQT
      size_t s = 0;
      while (s < n) {
        const int pq = seg[s] >> 4, tq = seg[s] & 15;
        if (pq != 0) return r.fail(pq == 1 ? RR_E_UNSUPPORTED : RR_E_PARSE, "jpeg: a 16-bit quantisation table");
        if (tq > 3 || s + 65 > n) return r.fail(RR_E_PARSE, "jpeg: a bad DQT segment");
        for (int k = 0; k < 64; k++) qt[tq][kZigzag[k]] = seg[s + 1 + k];
        have_q[tq] = true;
        s += 65;
      }
    } else if (m == 0xC0) {                                                       // SOF0
      if (have_sof) return r.fail(RR_E_PARSE, "jpeg: a second frame header");
      if (n < 6) return r.fail(RR_E_PARSE, "jpeg: a bad SOF0 segment");
      if (seg[0] != 8) return r.fail(RR_E_UNSUPPORTED, "jpeg: sample precision is not 8 bits");
      fr.H = (seg[1] << 8) | seg[2];
      fr.W = (seg[3] << 8) | seg[4];
      fr.ncomp = seg[5];
      if (fr.ncomp != 1 && fr.ncomp != 3)
        return r.fail(fr.ncomp == 4 || fr.ncomp == 2 ? RR_E_UNSUPPORTED : RR_E_PARSE, "jpeg: neither one nor three components");
      if (n != 6 + 3 * (size_t)fr.ncomp) return r.fail(RR_E_PARSE, "jpeg: a bad SOF0 segment");
      if (fr.W == 0) return r.fail(RR_E_PARSE, "jpeg: zero width");
      if (fr.H == 0) return r.fail(RR_E_UNSUPPORTED, "jpeg: the height comes in a DNL segment");
      int hv[3] = {0, 0, 0};
      for (int c = 0; c < fr.ncomp; c++) {
        fr.id[c] = seg[6 + 3 * c];
        hv[c] = seg[7 + 3 * c];
        fr.tq[c] = seg[8 + 3 * c];
        if (fr.tq[c] > 3 || (hv[c] >> 4) < 1 || (hv[c] >> 4) > 4 || (hv[c] & 15) < 1 || (hv[c] & 15) > 4)
          return r.fail(RR_E_PARSE, "jpeg: a bad component in SOF0");
        for (int d = 0; d < c; d++)
          if (fr.id[d] == fr.id[c]) return r.fail(RR_E_PARSE, "jpeg: two components share an identifier");
      }
      if (fr.ncomp == 1) fr.sampling = RR_JPEG_GREY;
      else if (hv[1] == 0x11 && hv[2] == 0x11 && hv[0] == 0x11) fr.sampling = RR_JPEG_444;
      else if (hv[1] == 0x11 && hv[2] == 0x11 && hv[0] == 0x21) fr.sampling = RR_JPEG_422;
      else if (hv[1] == 0x11 && hv[2] == 0x11 && hv[0] == 0x22) fr.sampling = RR_JPEG_420;
      else return r.fail(RR_E_UNSUPPORTED, "jpeg: sampling is not 4:4:4, 4:2:2 (2x1) or 4:2:0 (2x2)");
      if ((fr.sampling == RR_JPEG_422 || fr.sampling == RR_JPEG_420) && fr.W < 3)
        return r.fail(RR_E_UNSUPPORTED, "jpeg: subsampled chroma in a frame narrower than 3 pixels");
      have_sof = true;
    } else if (m == 0xC4) {                                                       // DHT
      size_t s = 0;
      while (s < n) {
        const int tc = seg[s] >> 4, th = seg[s] & 15;
        if (tc > 1 || th > 3 || s + 17 > n) return r.fail(RR_E_PARSE, "jpeg: a bad DHT segment");
        int nv = 0;
        for (int l = 0; l < 16; l++) nv += seg[s + 1 + l];
        if (nv > 256 || s + 17 + (size_t)nv > n) return r.fail(RR_E_PARSE, "jpeg: a bad DHT segment");
        if (!ht[tc][th].build(seg + s + 1, seg + s + 17, nv)) return r.fail(RR_E_PARSE, "jpeg: a Huffman table that is no prefix code");
        s += 17 + (size_t)nv;
      }
    } else if (m == 0xDD) {                                                       // DRI
      if (n != 2) return r.fail(RR_E_PARSE, "jpeg: a bad DRI segment");
      dri = (seg[0] << 8) | seg[1];
    } else if (m == 0xDA) {                                                       // SOS
      if (!have_sof) return r.fail(RR_E_PARSE, "jpeg: a scan before the frame header");
      if (n < 1 || n != 4 + 2 * (size_t)seg[0]) return r.fail(RR_E_PARSE, "jpeg: a bad SOS segment");
      if (seg[0] != fr.ncomp) return r.fail(RR_E_UNSUPPORTED, "jpeg: several scans (the first does not hold every component)");
      for (int c = 0; c < fr.ncomp; c++) {
        if (seg[1 + 2 * c] != fr.id[c]) return r.fail(RR_E_PARSE, "jpeg: the scan's components are not the frame's, in order");
        fr.td[c] = seg[2 + 2 * c] >> 4;
        fr.ta[c] = seg[2 + 2 * c] & 15;
        if (fr.td[c] > 3 || fr.ta[c] > 3 || !ht[0][fr.td[c]].defined || !ht[1][fr.ta[c]].defined)
          return r.fail(RR_E_PARSE, "jpeg: the scan names a Huffman table the file does not define");
        if (!have_q[fr.tq[c]]) return r.fail(RR_E_PARSE, "jpeg: a component names a quantisation table the file does not define");
      }
      if (seg[n - 3] != 0 || seg[n - 2] != 63 || seg[n - 1] != 0) return r.fail(RR_E_UNSUPPORTED, "jpeg: not a sequential scan of all 64 coefficients");
      break;
    } else if (m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8)) {
      return r.fail(RR_E_UNSUPPORTED, m == 0xC2 ? "jpeg: progressive (SOF2)"
                                                : (m == 0xC1 ? "jpeg: extended sequential (SOF1)" : "jpeg: a lossless, differential or arithmetic-coded file"));
    } else if (m == 0xDC) {
      return r.fail(RR_E_UNSUPPORTED, "jpeg: a DNL segment");
    } else if (!((m >= 0xE0 && m <= 0xEF) || m == 0xFE)) {                        // APPn / COM are skipped
      return r.fail(RR_E_UNSUPPORTED, "jpeg: a marker outside the baseline subset");
    }
  }
  Geom g;
  if (!geom_of(fr.W, fr.H, fr.sampling, g)) return r.fail(RR_E_PARSE, "jpeg: bad frame size");
  if (fr.want_W && (fr.W != fr.want_W || fr.H != fr.want_H)) return r.fail(RR_E_ARG, "jpeg: the file is not of the expected size");
  if (hdr) {
    memset(hdr, 0, sizeof *hdr);
    hdr->magic = RR_JPEG_MAGIC;
    hdr->W = fr.W;
    hdr->H = fr.H;
    hdr->sampling = fr.sampling;
    hdr->components = fr.ncomp;
    for (int c = 0; c < fr.ncomp; c++) memcpy(hdr->q[c], qt[fr.tq[c]], 128);
  }
  if (!coef) return RR_OK;                             // (rr_jpeg_info vouches for the kind of file, not for its data)
  if (cap_blocks < g.nblocks) return r.fail(RR_E_ARG, "jpeg: the record does not fit the buffer");
  // ---- the scan: MCU by MCU, a component's hs x vs blocks in raster order inside the MCU ----
  BitReader br;
  br.p = b + p;
  br.end = b + size;
  int32_t pred[3] = {0, 0, 0};
  const int64_t mcus = (int64_t)g.mw * g.mh;
  int32_t until_rst = dri, rst_no = 0;
  for (int64_t mi = 0; mi < mcus; mi++) {
    if (dri && until_rst == 0) {                        // a restart interval ends here: byte-align, RSTn in sequence, predictions reset
      if (br.overrun()) return r.fail(RR_E_PARSE, "jpeg: the entropy-coded data ends early");
      const uint8_t* q = br.p;
      if (q >= br.end || *q != 0xFF) return r.fail(RR_E_PARSE, "jpeg: a restart marker is missing");
      while (q < br.end && *q == 0xFF) q++;
      if (q >= br.end || *q != 0xD0 + rst_no) return r.fail(RR_E_PARSE, "jpeg: a restart marker is missing or out of sequence");
      br.p = q + 1;
      br.restart();
      rst_no = (rst_no + 1) & 7;
      until_rst = dri;
      pred[0] = pred[1] = pred[2] = 0;
    }
    until_rst--;
    const int my = (int)(mi / g.mw), mx = (int)(mi % g.mw);
    for (int c = 0; c < g.ncomp; c++) {
      const int ch = c ? 1 : g.hs, cv = c ? 1 : g.vs, bw = g.pw[c] / 8;
      const HuffTable &dc = ht[0][fr.td[c]], &ac = ht[1][fr.ta[c]];
      for (int by = 0; by < cv; by++)
        for (int bx = 0; bx < ch; bx++) {
          int16_t* blk = coef + (g.blk0[c] + (int64_t)(my * cv + by) * bw + (mx * ch + bx)) * 64;
          memset(blk, 0, 128);
          const int t = decode_symbol(br, dc);
          if (t < 0) return r.fail(RR_E_PARSE, "jpeg: a Huffman code that is not in the table");
          if (t > 15) return r.fail(RR_E_PARSE, "jpeg: a DC category above 15");
          pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)receive_extend(br, t));
          blk[0] = (int16_t)(uint16_t)(uint32_t)pred[c];
          int k = 1;
          while (k < 64) {
            br.fill();
            const int32_t fa = ac.fast_ac[br.peek(9)];
            if (fa) {                                   // run, code and magnitude in one look-up
              k += (fa >> 4) & 15;
              if (k > 63) return r.fail(RR_E_PARSE, "jpeg: a zero run past coefficient 63");
              blk[kZigzag[k++]] = (int16_t)(fa >> 8);
              br.skip(fa & 15);
              continue;
            }
            const int rs = decode_symbol(br, ac);
            if (rs < 0) return r.fail(RR_E_PARSE, "jpeg: a Huffman code that is not in the table");
            const int run = rs >> 4, s = rs & 15;
            if (!s) {
              if (run != 15) break;                     // EOB
              k += 16;                                  // ZRL
              if (k > 64) return r.fail(RR_E_PARSE, "jpeg: a zero run past coefficient 63");
              continue;
            }
            k += run;
            if (k > 63) return r.fail(RR_E_PARSE, "jpeg: a zero run past coefficient 63");
            blk[kZigzag[k]] = (int16_t)receive_extend(br, s);
            k++;
          }
          if (br.overrun()) return r.fail(RR_E_PARSE, "jpeg: the entropy-coded data ends early");
        }
    }
  }
  // ---- behind the scan: EOI (fill bytes allowed); a second scan or more data is not this decoder's file ----
  const uint8_t* q = br.p;
  if (q >= br.end || *q != 0xFF) return r.fail(RR_E_PARSE, "jpeg: no EOI marker behind the scan");
  while (q < br.end && *q == 0xFF) q++;
  if (q >= br.end) return r.fail(RR_E_PARSE, "jpeg: no EOI marker behind the scan");
  if (*q == 0xDA || *q == 0xC4 || *q == 0xDB) return r.fail(RR_E_UNSUPPORTED, "jpeg: several scans");
  if (*q != 0xD9) return r.fail(RR_E_PARSE, "jpeg: no EOI marker behind the scan");
  return RR_OK;
}

// planes (g.nblocks * 64 bytes) of a record's body: every block through jpeg_idct_islow into its place in its component's plane
inline void record_planes(const rr_jpeg_header& hdr, const Geom& g, const int16_t* coef, uint8_t* planes) {
  uint8_t blk[64];
  for (int c = 0; c < g.ncomp; c++) {
    const int bw = g.pw[c] / 8, bh = g.ph[c] / 8;
    uint8_t* pl = planes + g.blk0[c] * 64;
    for (int by = 0; by < bh; by++)
      for (int bx = 0; bx < bw; bx++) {
        jpeg_idct_islow(coef + (g.blk0[c] + (int64_t)by * bw + bx) * 64, hdr.q[c], blk);
        for (int y = 0; y < 8; y++) memcpy(pl + ((int64_t)by * 8 + y) * g.pw[c] + bx * 8, blk + y * 8, 8);
      }
  }
}

}  // namespace rrjpeg
