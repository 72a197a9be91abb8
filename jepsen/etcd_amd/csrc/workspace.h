// workspace.h — one device allocation carved into the arrays of a call.
//
// A side checker's driver writes its layout once, as a function that takes
// a Carver and assigns every array's pointer where the kernels look for it
// (the fields of its Ws, a few pointers beside it), and runs it twice: over
// a null base, which only adds the sizes up, then, once ensure() has made
// the arena that large, over the arena.  An array starts on a 256-byte
// boundary of the arena and has at least 256 bytes of its own, also when its
// count is 0: what a buffer of its own from ensure() would give it.
// Host-only, nothing of HIP: tests/workspace_main.cpp compiles it with g++.
#pragma once
#include <stddef.h>

namespace lcrt __attribute__((visibility("hidden"))) {

inline size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

struct Carver {
  char *base = nullptr;  // null: the sizing pass, and every take() is null
  size_t size = 0;       // the bytes taken so far
  template <class T>
  T *take(size_t count) {
    char *p = base ? base + size : nullptr;
    const size_t bytes = count * sizeof(T);
    size += up256(bytes < 256 ? 256 : bytes);
    return reinterpret_cast<T *>(p);
  }
};

}  // namespace lcrt
