// The one bump allocator of the library's workspaces.  An entry point writes its layout ONCE, as a carve over an SfArena: the size query runs it
// over a NULL base (it only counts), the call over the caller's `ws`, so the two cannot disagree about a buffer.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct SfArena {
  char* base;        // `ws` aligned up to 256 bytes (at most 255 bytes of the entry point's slack), or NULL: count only
  size_t left;       // bytes the caller's limit still allows
  size_t used = 0;
  bool ok = true;    // false once a take did not fit the limit (that take and every later one return NULL)
  explicit SfArena(void* ws, size_t limit = ~(size_t)0) : base((char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255)), left(limit) {
    const size_t skip = (size_t)(base - (char*)ws);
    left = left > skip ? left - skip : 0;
  }
  // n elements of T: the pointer (NULL when counting or out of room); advances by n * sizeof(T) rounded up to 256 bytes (64 floats)
  template <class T = float>
  T* take(size_t n) {
    const size_t b = (n * sizeof(T) + 255) & ~(size_t)255;
    if (!ok || b > left) return ok = false, nullptr;
    T* r = base ? (T*)(base + used) : nullptr;
    used += b, left -= b;
    return r;
  }
  size_t bytes() const { return used; }   // carved so far: a size query returns this + the entry point's slack constant
};
