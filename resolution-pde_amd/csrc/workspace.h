// The caller's workspace: one bump allocator that both carves and measures.  An entry describes its
// scratch once, as a layout: a struct whose constructor takes pieces from an Arena&.  The entry builds the layout on
// Arena(ws, ws_bytes) and claims it; its *_ws_bytes query builds the same layout on a measuring arena, so the two
// cannot disagree.
#pragma once
#include "rpde_internal.h"

namespace rpde {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t arena_bytes(size_t floats) { return align_up(floats * sizeof(float), 256); }

// bump allocator of 256-byte aligned pieces.  Arena(ws, n) carves the caller's n bytes and fails on a null ws or a
// short n; Arena() has no base and only measures: take returns null and always succeeds.  Either way `used` ends as
// the bytes the pieces need
struct Arena {
  char* base; size_t size, used; bool measuring, failed;
  Arena() : base(nullptr), size(0), used(0), measuring(true), failed(false) {}
  Arena(void* p, size_t n) : base(static_cast<char*>(p)), size(n), used(0), measuring(false), failed(false) {}
  float* take(size_t floats) {
    const size_t at = used;
    used += arena_bytes(floats);
    if (measuring) return nullptr;
    if (!base || used > size) { failed = true; return nullptr; }
    return reinterpret_cast<float*>(base + at);
  }
  bool ok() const { return !failed; }
};

// bytes of layout L for these dims: L built on a measuring arena
template <class L, class... A>
inline size_t ws_measure(const A&... dims) {
  Arena ar;
  L layout(ar, dims...);
  (void)layout;
  return ar.used;
}
inline size_t ws_max(size_t a, size_t b) { return a > b ? a : b; }

// the verdict on a carved layout, before anything is planned or launched.  `what`: the entry's name, a literal or a
// variable
#define RPDE_CLAIM_WS(what, ar, given)                                                                              \
  do {                                                                                                              \
    if (!(ar).ok()) {                                                                                               \
      ::rpde::set_error("%s: workspace too small (%zu bytes, needs %zu)", what, (size_t)(given), (ar).used);        \
      return RPDE_ERR_WORKSPACE;                                                                                    \
    }                                                                                                               \
  } while (0)

// what an entry does with (ws, given): `const L wk` carved from them with these dims, or the verdict
#define RPDE_CARVE(what, L, wk, ws, given, ...) \
  ::rpde::Arena wk##_arena(ws, given);          \
  const L wk(wk##_arena, __VA_ARGS__);          \
  RPDE_CLAIM_WS(what, wk##_arena, given)

}  // namespace rpde
