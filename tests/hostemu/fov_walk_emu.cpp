// tests/hostemu/fov_walk_emu.cpp -- TEST INFRASTRUCTURE ONLY.
//
// k_fov_dda's polygon walk (rr_device.h fov_walk_make_records + FovWalk: chained 16-byte records, an edge switch that is
// a hand-over) built with g++ and run against the rules it walks -- fov_rowspan and, where it applies, fov_rowspan_cv --
// and beside the walker it replaced (DdaCursors, kept as the reference statement).  tests/test_fov_walk_host.py drives it.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "rr_device.h"

using namespace rr;

namespace {

// rows of [0, He) on which a walk's (a <= b, a, b) differs from the rule
template <class ROW>
int rows_off_the_rule(const int32_t* px, const int32_t* py, int n, int He, int We, int rule, int ytop, int ybot, ROW&& row) {
  int bad = 0;
  for (int y = 0; y < He; y++) {
    int lo = 1 << 30, hi = -(1 << 30);
    if (y >= ytop && y <= ybot) row(y, lo, hi);
    const int a = imax(lo, 0), b = imin(hi, We - 1);
    int xl, xr;
    const bool any = rule == 1 ? fov_rowspan_cv(px, py, n, y, We, xl, xr) : fov_rowspan(px, py, n, y, We, xl, xr);
    if (any != (a <= b) || (any && (xl != a || xr != b))) bad++;
  }
  return bad;
}

// the new walk and the old one on one polygon: -1 (both) where the kernel would not walk it
int walk_check(const int32_t* px, const int32_t* py, int n, int He, int We, int rule, int* bad_old) {
  *bad_old = -1;
  if (poly_row_turns(py, n) > 2) return -1;
  if (rule == 1 && !fov_fill_rule_cv_applies(px, py, n, n, He, We)) return -1;
  int ktop = 0, ytop = py[0], ybot = py[0];
  for (int k = 1; k < n; k++) {
    if (py[k] < ytop) { ytop = py[k]; ktop = k; }          // (k_fov_vertices: the first vertex of the top row)
    if (py[k] > ybot) ybot = py[k];
  }
  const bool cv = rule == 1;
  // the records exactly as the kernel's prologue makes them: the same function, the chain's n + 1 positions; a position
  // nobody wrote holds a pattern no row may come to depend on
  std::vector<uint32_t> chain(4 * (size_t)(n + 1), 0xdeadbeefu);
  int written = 0, out_of_chain = 0;
  auto vtx = [&](int k) { return (uint32_t)(px[k] & 0xffff) | ((uint32_t)(py[k] & 0xffff) << 16); };
  auto store = [&](int pos, const uint32_t r[4]) {
    if (pos < 0 || pos > n) { out_of_chain++; return; }
    for (int q = 0; q < 4; q++) chain[4 * (size_t)pos + q] = r[q];
    written++;
  };
  const int n_pos = fov_walk_make_records(vtx, n, ktop, cv, store);
  if (out_of_chain || n_pos != written || n_pos < 1 || n_pos > n + 1) return 1 << 20;
  int fetched_outside = 0;
  auto rec = [&](int pos, uint32_t r[4]) {
    if (pos < 0 || pos >= n_pos) { fetched_outside++; pos = 0; }
    for (int q = 0; q < 4; q++) r[q] = chain[4 * (size_t)pos + q];
  };
  FovWalk<decltype(rec)> walk;
  walk.init(rec, n_pos, ytop, cv);
  int bad = rows_off_the_rule(px, py, n, He, We, rule, ytop, ybot, [&](int y, int& lo, int& hi) { walk.row(rec, y, lo, hi); });
  if (fetched_outside) bad += 1 << 20;

  std::vector<uint32_t> recs(4 * (size_t)n);                 // the walker before: a record per edge {k, k + 1}
  for (int k = 0; k < n; k++) {
    const int j = k + 1 == n ? 0 : k + 1;
    const bool swp = py[j] < py[k];
    dda_edge_record(swp ? px[j] : px[k], swp ? py[j] : py[k], swp ? px[k] : px[j], swp ? py[k] : py[j], cv, &recs[4 * (size_t)k]);
  }
  auto orec = [&](int k, uint32_t r[4]) { for (int q = 0; q < 4; q++) r[q] = recs[4 * (size_t)k + q]; };
  DdaCursors<decltype(orec)> cur;
  cur.init(orec, n, ktop, (uint32_t)px[ktop] | ((uint32_t)py[ktop] << 16));
  *bad_old = rows_off_the_rule(px, py, n, He, We, rule, ytop, ybot, [&](int y, int& lo, int& hi) { cur.row(orec, y, lo, hi); });
  return bad;
}

struct Rng {                                                 // xorshift64*: the test needs variety, not a particular stream
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
  int randint(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo)); }      // [lo, hi)
};

}  // namespace

extern "C" {

// one polygon under one rule (0: the span rule, 1: OpenCV's where it applies): rows on which the new walk differs from the
// rule; *bad_old: the same count for DdaCursors.  -1 / -1: not monotone, or rule 1 does not apply.
int fov_walk_check(const int32_t* px, const int32_t* py, int n, int He, int We, int rule, int32_t* bad_old) {
  int o = -1;
  const int b = walk_check(px, py, n, He, We, rule, &o);
  *bad_old = o;
  return b;
}

// `trials` random monotone polygons with many ties, test_thread_per_drop_spans_equal_the_rule's generator in C++ (a top
// vertex, up to 8 vertices down one side, a bottom vertex, up to 8 up the other, rolled anywhere in the loop), either
// orientation, under both rules.  border: vertices may lie on row He and column We (off the map: rule 1 does not apply),
// as that generator has them; 0 keeps every vertex on the map, which also keeps den <= He - 1 and |dx| <= We - 1.
// out[0] polygons walked under rule 0, out[1] under rule 1, out[2] rows off the rule (new walk), out[3] rows off (DdaCursors),
// out[4] polygons the generator made that are not monotone (none), out[5] largest den, out[6] largest |dx|.
int fov_walk_random(uint64_t seed, int trials, int He, int We, int border, int64_t* out) {
  Rng g{seed * 2654435761ull + 88172645463325252ull};
  for (int q = 0; q < 7; q++) out[q] = 0;
  std::vector<int32_t> px, py, qx, qy;
  for (int t = 0; t < trials; t++) {
    const int ymax = border ? He : He - 1, xmax = border ? We : We - 1;
    const int n_l = g.randint(1, 9), n_r = g.randint(1, 9);
    int y_top = g.randint(0, ymax + 1), y_bot = g.randint(0, ymax + 1);
    if (y_top > y_bot) std::swap(y_top, y_bot);
    if (t % 4 == 3) y_bot = std::min(y_bot, y_top + g.randint(0, 12));      // a quarter of them short: shared rows, den = 1 edges
    std::vector<int32_t> ys_l(n_l), ys_r(n_r);
    for (auto& v : ys_l) v = g.randint(y_top, y_bot + 1);
    for (auto& v : ys_r) v = g.randint(y_top, y_bot + 1);
    std::sort(ys_l.begin(), ys_l.end());
    std::sort(ys_r.begin(), ys_r.end(), [](int a, int b) { return a > b; });
    px.clear(); py.clear();
    px.push_back(g.randint(0, We)); py.push_back(y_top);
    for (int k = 0; k < n_l; k++) { px.push_back(g.randint(0, We / 2)); py.push_back(ys_l[k]); }
    px.push_back(g.randint(0, We)); py.push_back(y_bot);
    for (int k = 0; k < n_r; k++) { px.push_back(g.randint(We / 2, xmax + 1)); py.push_back(ys_r[k]); }
    const int n = (int)px.size(), roll = g.randint(0, n);
    const bool flip = g.next() & 1u;
    qx.resize(n); qy.resize(n);
    for (int k = 0; k < n; k++) {
      const int src = flip ? n - 1 - k : k;
      qx[(k + roll) % n] = px[src];
      qy[(k + roll) % n] = py[src];
    }
    for (int k = 0; k < n; k++) {
      const int j = k + 1 == n ? 0 : k + 1;
      out[5] = std::max<int64_t>(out[5], std::abs(qy[j] - qy[k]));
      out[6] = std::max<int64_t>(out[6], std::abs(qx[j] - qx[k]));
    }
    for (int rule = 0; rule < 2; rule++) {
      int o = -1;
      const int b = walk_check(qx.data(), qy.data(), n, He, We, rule, &o);
      if (b < 0) {
        if (rule == 0) out[4]++;
        continue;
      }
      out[rule]++;
      out[2] += b;
      out[3] += o;
    }
  }
  return 0;
}

}  // extern "C"
