// The memory owner of a context (csrc/rr_mem.h) over a malloc backend, under AddressSanitizer + UndefinedBehaviorSanitizer
// with leak detection ON: the backend counts live blocks and every free per block, and can be told to fail its k-th
// allocation.  Checks (tests/test_codec_sanitized.py reads the last line):
//   (a) allocations, regrows, early frees, release_all: nothing live afterwards, every block freed exactly once
//   (b) a regrow frees the old block before it returns: the live count does not rise
//   (c) reserve with need <= cap allocates nothing (and does not call the synchronise)
//   (d) a failure injected at the first, a middle and the last allocation of a device + pinned pair and of a plain buffer:
//       null pointers, capacity 0, nothing stale recorded; the next reserve succeeds and the live count is right
//   (e) the slack formulas of the library's sites (exact, x1.5, x1.5 + 4096, 2n + 64) arrive at the backend unchanged
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "rr_mem.h"

namespace {

struct MallocBackend {
  std::map<void*, int> frees;          // per block ever handed out at this address since its last allocation: times freed
  std::map<void*, bool> pinned;
  long live_dev = 0, live_pin = 0, allocs = 0, fail_at = -1, wrong = 0;
  size_t last_bytes = 0;
  int get(void** p, size_t bytes, bool pin) {
    if (allocs++ == fail_at) {
      *p = nullptr;
      return 2;                        // ("out of memory")
    }
    *p = malloc(bytes);
    memset(*p, 0x5a, bytes);           // the whole block is ours to write
    frees[*p] = 0;
    pinned[*p] = pin;
    (pin ? live_pin : live_dev)++;
    last_bytes = bytes;
    return 0;
  }
  int put(void* p, bool pin) {
    auto it = frees.find(p);
    if (it == frees.end() || it->second != 0 || pinned[p] != pin) {
      wrong++;                         // a foreign block, a second free, or the wrong kind of free
      return 1;
    }
    it->second = 1;
    (pin ? live_pin : live_dev)--;
    free(p);
    return 0;
  }
  int dev_alloc(void** p, size_t bytes) { return get(p, bytes, false); }
  int dev_free(void* p) { return put(p, false); }
  int pin_alloc(void** p, size_t bytes) { return get(p, bytes, true); }
  int pin_free(void* p) { return put(p, true); }
};

using Owner = rrmem::Owner<MallocBackend>;

int g_wrong = 0, g_checks = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    g_checks++;                                                  \
    if (!(cond)) {                                               \
      g_wrong++;                                                 \
      printf("line %d: %s\n", __LINE__, #cond);                  \
    }                                                            \
  } while (0)

bool stats_are(const Owner& o, long nd, long bd, long np, long bp) {
  int64_t s[4];
  o.stats(s);
  return s[0] == nd && (bd < 0 || s[1] == bd) && s[2] == np && (bp < 0 || s[3] == bp) && o.backend.live_dev == nd && o.backend.live_pin == np;
}

int g_syncs = 0;
struct CountSync {
  int operator()() const { return g_syncs++, 0; }
};

void check_lifecycle() {               // (a), (b)
  Owner o;
  double *a = nullptr, *b = nullptr;
  int32_t* c = nullptr;
  char* h = nullptr;
  CHECK(o.alloc(a, 100) && o.alloc(b, 0) && o.alloc(c, 7) && o.alloc_pinned(h, 33));
  CHECK(stats_are(o, 3, 100 * 8 + 1 * 8 + 7 * 4, 1, 33));           // (count 0 allocates one element)
  double* const a0 = a;
  CHECK(o.alloc(a, 1000));                                          // regrow: the old block first
  CHECK(o.backend.frees[a0] == 1 || a == a0);                       // (malloc may hand the same address out again)
  CHECK(stats_are(o, 3, 1000 * 8 + 8 + 28, 1, 33));
  CHECK(o.alloc_pinned(h, 5) && stats_are(o, 3, -1, 1, 5));
  o.free(b);
  CHECK(b == nullptr && stats_are(o, 2, 1000 * 8 + 28, 1, 5));
  o.free(b);                                                        // a null pointer: nothing
  o.free(h);                                                        // free() finds a pinned block too
  CHECK(h == nullptr && stats_are(o, 2, -1, 0, 0));
  int foreign = 0;
  int* fp = &foreign;
  o.free(fp);                                                       // not ours: left alone
  CHECK(o.backend.wrong == 0 && stats_are(o, 2, -1, 0, 0));
  std::vector<void*> blocks;                                        // the noise blocks / ext blobs of the library
  for (int k = 0; k < 5; k++) {
    char* blk = nullptr;
    CHECK(o.alloc(blk, 64 + k));
    blocks.push_back(blk);
  }
  CHECK(stats_are(o, 7, -1, 0, 0));
  for (void*& blk : blocks) o.free(blk);
  CHECK(stats_are(o, 2, 1000 * 8 + 28, 0, 0));
  o.release_all();
  CHECK(stats_are(o, 0, 0, 0, 0) && o.backend.wrong == 0);
  o.release_all();                                                  // twice: nothing left to free
  CHECK(o.backend.wrong == 0);
  for (const auto& f : o.backend.frees) CHECK(f.second == 1);       // every block exactly once
}

void check_reserve() {                 // (b), (c), (e)
  Owner o;
  rrmem::Buf<int32_t> buf;
  rrmem::PinnedBuf<char> ring;
  rrmem::MirrorBuf<double> list;
  g_syncs = 0;
  CHECK(o.reserve(buf, 10, 0, CountSync()) && buf.cap == 10 && o.backend.last_bytes == 40 && g_syncs == 1);       // exact
  const long before = o.backend.allocs;
  CHECK(o.reserve(buf, 10, 0, CountSync()) && o.reserve(buf, 3, 999, CountSync()) && o.backend.allocs == before && g_syncs == 1);
  const size_t bytes = 1000;
  CHECK(o.reserve(ring, bytes, bytes + bytes / 2 + 4096) && ring.cap == 5596 && o.backend.last_bytes == 5596);   // x1.5 + 4096
  CHECK(o.reserve(ring, 5596, 5596 + 5596 / 2 + 4096) && o.backend.allocs == before + 1);
  rrmem::Buf<char> block;
  CHECK(o.reserve(block, bytes, bytes + bytes / 2) && block.cap == 1500 && o.backend.last_bytes == 1500);          // x1.5
  const size_t n = 21;
  CHECK(o.reserve(list, n, n * 2 + 64) && list.cap == 106 && o.backend.last_bytes == 106 * 8 && list.d && list.h); // 2n + 64
  CHECK(stats_are(o, 3, 40 + 1500 + 106 * 8, 2, 5596 + 106 * 8));
  CHECK(o.reserve(list, 107, 107 * 2 + 64) && list.cap == 278 && stats_are(o, 3, 40 + 1500 + 278 * 8, 2, 5596 + 278 * 8));   // old pair gone
  CHECK(o.reserve(buf, 11, 0) && buf.cap == 11 && stats_are(o, 3, 44 + 1500 + 278 * 8, 2, -1));
  struct FailSync {
    int operator()() const { return 7; }
  };
  int32_t* const kept = buf.p;
  CHECK(!o.reserve(buf, 12, 0, FailSync()) && o.last_error == 7 && buf.p == kept && buf.cap == 11);      // the wait failed: untouched
  buf.p[10] = 1;
  ring.p[5595] = 1;
  list.d[277] = list.h[277] = 1.0;                                  // the last element of each is inside its block
}

// (d): allocation k of a regrow of a buffer of kind B fails; one such buffer holds dev_blocks device and pin_blocks pinned blocks
template <class B>
void check_failure(int k, long dev_blocks, long pin_blocks) {
  Owner o;
  B b;
  char* other = nullptr;
  CHECK(o.alloc(other, 16));                                        // somebody else's block stays through it all
  CHECK(o.reserve(b, 8, 8) && b.cap == 8 && stats_are(o, 1 + dev_blocks, -1, pin_blocks, -1));
  o.backend.fail_at = o.backend.allocs + k;
  CHECK(!o.reserve(b, 9, 20) && o.last_error == 2);
  CHECK(b.cap == 0 && stats_are(o, 1, 16, 0, 0));                   // nothing of b is recorded, nothing of it is live
  B empty;
  CHECK(memcmp(&b, &empty, sizeof b) == 0);                         // every pointer null
  CHECK(o.reserve(b, 2, 2) && b.cap == 2 && stats_are(o, 1 + dev_blocks, -1, pin_blocks, -1));    // smaller than before: still a fresh start
  o.backend.fail_at = o.backend.allocs;                             // and a failure of the very first allocation of a buffer
  B c;
  CHECK(!o.reserve(c, 1, 1) && c.cap == 0 && memcmp(&c, &empty, sizeof c) == 0 && stats_are(o, 1 + dev_blocks, -1, pin_blocks, -1));
  CHECK(o.reserve(c, 1, 1) && stats_are(o, 1 + 2 * dev_blocks, -1, 2 * pin_blocks, -1));
  double* p = nullptr;
  CHECK(o.alloc(p, 4));
  o.backend.fail_at = o.backend.allocs;
  CHECK(!o.alloc(p, 8) && p == nullptr && stats_are(o, 1 + 2 * dev_blocks, -1, 2 * pin_blocks, -1));   // alloc: null, old block gone
  CHECK(o.backend.wrong == 0);
}                                      // (~Owner releases the rest: the leak checker sees what it misses)

}  // namespace

int main() {
  check_lifecycle();
  check_reserve();
  check_failure<rrmem::Buf<float>>(0, 1, 0);                        // a plain buffer has one allocation: first = middle = last
  check_failure<rrmem::PinnedBuf<char>>(0, 0, 1);
  check_failure<rrmem::MirrorBuf<int64_t>>(0, 1, 1);                // the pair: its device block fails ...
  check_failure<rrmem::MirrorBuf<int64_t>>(1, 1, 1);                // ... or its pinned mirror, the device block already there
  // a group as the library grows them (several arrays, one capacity record): first, middle and last array failing
  for (int k = 0; k < 3; k++) {
    Owner o;
    double* arr[3] = {nullptr, nullptr, nullptr};
    for (auto& a : arr) CHECK(o.alloc(a, 10));
    o.backend.fail_at = o.backend.allocs + k;
    bool ok = true;
    for (auto& a : arr) ok = ok && o.alloc(a, 20);
    CHECK(!ok && arr[k] == nullptr && stats_are(o, 2, -1, 0, 0));
    for (auto& a : arr) CHECK(o.alloc(a, 20));                      // the full reallocation that follows
    CHECK(stats_are(o, 3, 3 * 20 * 8, 0, 0) && o.backend.wrong == 0);
  }
  printf("mem_owner: checks %d, wrong %d\n", g_checks, g_wrong);
  return g_wrong ? 1 : 0;
}
