// One owner for the device and pinned memory of a context.  Every block a context allocates is recorded here, so
// the context is torn down by release_all() and no buffer has to be named twice.  The owner is written against a backend of four
// functions -- rainhip.hip gives it the HIP calls, tests/sanitize/mem_owner.cpp gives it malloc:
//   int dev_alloc(void** p, size_t bytes);  int dev_free(void* p);  int pin_alloc(void** p, size_t bytes);  int pin_free(void* p);
// each returning 0 or the backend's error code (kept in last_error).  One backend allocation per array: nothing is pooled or merged.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rrmem {

// grow-only buffers: a device array, a pinned array, or a device array with its pinned mirror, and the elements they hold
template <class T>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;
};
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
};
template <class T>
struct MirrorBuf {
  T *d = nullptr, *h = nullptr;
  size_t cap = 0;
};

template <class Backend>
class Owner {
 public:
  Backend backend;
  int last_error = 0;      // the backend's code of the allocation that failed last

  Owner() = default;
  Owner(const Owner&) = delete;
  Owner& operator=(const Owner&) = delete;
  ~Owner() { release_all(); }

  // *p is freed and forgotten, then max(count, 1) elements are allocated and recorded; on failure p is null
  template <class T>
  bool alloc(T*& p, size_t count) { return replace(dev_, p, count, false); }
  template <class T>
  bool alloc_pinned(T*& p, size_t count) { return replace(pin_, p, count, true); }

  // one block early, device or pinned; a null or foreign pointer is left alone
  template <class T>
  void free(T*& p) {
    if (!drop(dev_, (void*)p, false)) drop(pin_, (void*)p, true);
    p = nullptr;
  }

  void release_all() {
    for (const Block& b : dev_) backend.dev_free(b.p);
    for (const Block& b : pin_) backend.pin_free(b.p);
    dev_.clear();
    pin_.clear();
  }

  // live device blocks, their bytes, live pinned blocks, their bytes
  void stats(int64_t out[4]) const {
    out[0] = (int64_t)dev_.size();
    out[2] = (int64_t)pin_.size();
    out[1] = out[3] = 0;
    for (const Block& b : dev_) out[1] += (int64_t)b.bytes;
    for (const Block& b : pin_) out[3] += (int64_t)b.bytes;
  }

  // Room for `need` elements: nothing when the buffer has it; otherwise before_free() (the caller's synchronise; a non-zero
  // answer ends the call with the buffer untouched), the capacity to zero, the old blocks freed and `want` (the site's own
  // slack formula; need where it is smaller) elements allocated.  A failure leaves null pointers and capacity 0, so the next
  // call starts afresh.
  struct NoSync {
    int operator()() const { return 0; }
  };
  template <class B, class Sync = NoSync>
  bool reserve(B& b, size_t need, size_t want, Sync before_free = Sync()) {
    if (need <= b.cap) return true;
    if ((last_error = before_free()) != 0) return false;
    b.cap = 0;
    if (!regrow(b, want < need ? need : want)) {
      release(b);
      return false;
    }
    b.cap = want < need ? need : want;
    return true;
  }

 private:
  struct Block {
    void* p;
    size_t bytes;
  };
  std::vector<Block> dev_, pin_;

  bool drop(std::vector<Block>& v, void* p, bool pinned) {
    if (!p) return false;
    for (size_t k = 0; k < v.size(); k++)
      if (v[k].p == p) {
        v[k] = v.back();
        v.pop_back();
        pinned ? backend.pin_free(p) : backend.dev_free(p);
        return true;
      }
    return false;
  }
  template <class T>
  bool replace(std::vector<Block>& v, T*& p, size_t count, bool pinned) {
    drop(v, (void*)p, pinned);
    p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    void* q = nullptr;
    const int e = pinned ? backend.pin_alloc(&q, bytes) : backend.dev_alloc(&q, bytes);
    if (e != 0 || !q) {
      last_error = e;
      return false;
    }
    v.push_back(Block{q, bytes});
    p = static_cast<T*>(q);
    return true;
  }
  template <class T>
  bool regrow(Buf<T>& b, size_t n) { return alloc(b.p, n); }
  template <class T>
  bool regrow(PinnedBuf<T>& b, size_t n) { return alloc_pinned(b.p, n); }
  template <class T>
  bool regrow(MirrorBuf<T>& b, size_t n) {
    free(b.d);                         // both old blocks go before either new one comes
    free(b.h);
    return alloc(b.d, n) && alloc_pinned(b.h, n);
  }
  template <class T>
  void release(Buf<T>& b) { free(b.p); }
  template <class T>
  void release(PinnedBuf<T>& b) { free(b.p); }
  template <class T>
  void release(MirrorBuf<T>& b) {
    free(b.d);
    free(b.h);
  }
};

}  // namespace rrmem
