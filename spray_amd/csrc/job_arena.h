// job_arena.h -- the scratch of a batched slot call (refit, build,
// isosurface): one device buffer laid out by typed takes, with a pinned host
// mirror of its head, the tables the host fills and reads.  No HIP header:
// the storage is arena_reserve / arena_release / arena_copy (rt_ctx.h).
#pragma once

#include <cassert>
#include <cstddef>
#include <cstdint>

namespace spray_rt {
namespace detail {

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// count elements of T at byte `off` of a layout (SIZE_MAX: nothing taken).
template <class T>
struct Take {
  size_t off = SIZE_MAX;
  explicit operator bool() const { return off != SIZE_MAX; }
  T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};
// A take inside the mirrored head: the only kind with a host side.
template <class T>
struct HeadTake : Take<T> {};

// Takes in order, each align256(count * sizeof(T)) bytes; owns nothing.
struct Layout {
  size_t used = 0;  // the running total == mark()
  template <class T>
  Take<T> take(size_t count) {
    Take<T> t;
    t.off = used;
    used += align256(count * sizeof(T));
    return t;
  }
  size_t mark() const { return used; }
};

struct JobArena : Layout {
  void* d = nullptr;  // device buffer, d_cap bytes (grows through ensure)
  size_t d_cap = 0;
  void* h = nullptr;  // pinned mirror of [0, head), h_cap bytes
  size_t h_cap = 0;
  size_t head = 0;  // where the last mirrored take of the call laid out ends

  void reset() { used = head = 0; }
  template <class T>
  HeadTake<T> take_head(size_t count) {
    assert(head == used);  // the head is a prefix
    HeadTake<T> t;
    t.off = take<T>(count).off;
    head = used;
    return t;
  }
  template <class T>
  T* dev(Take<T> t) const { return t.at(d); }
  template <class T>
  T* host(HeadTake<T> t) const { return t.at(h); }
};

}  // namespace detail
}  // namespace spray_rt
