// counted.h — the counted-class layout rule (include/lincheck.h,
// lc_counted_plan / LC_FLAG_COUNTED_CLASSES), shared by the host planner
// (plan_host.h) and the counted tier (check_kernel.hip): both must cut a
// configuration's 64-bit mask into the same fields.
//
// Classes: the distinct (f, value, expected, version) among a key's crashed
// writes/CAS (ret == LC_INF), in order of first call.  Class c with m_c
// members owns a field of width_c = floor(log2(m_c)) + 1 bits holding the
// absolute number of its members linearized; fields are packed from bit 63
// downward in class order (shift_c = 64 - sum of width_0..width_c).  Class c
// also owns lane 63 - c (its precondition and effect).  What is left below
// both, slots = min(64 - sum of widths, 64 - n_classes), are one-bit window
// slots for every other open op.  A key fits with at most kCountedMaxClasses
// classes and at least one slot.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LCCOUNT_FN __host__ __device__ inline
#else  // the host planner under g++ (plan_host.h): plain functions
#define LCCOUNT_FN inline
#endif
#include <stdint.h>

namespace lccount {

constexpr int kCountedMaxClasses = 16;

// A version as the device reads it (records.h decode): one outside
// [-1, 2^31-2] is a version no state reaches, saturated to 2^31-2.
LCCOUNT_FN int64_t counted_version(int64_t v) {
  return (v < -1 || v > 0x7FFFFFFE) ? 0x7FFFFFFE : v;
}

// floor(log2(members)) + 1 for members >= 1.
LCCOUNT_FN int counted_width(int64_t members) {
  int w = 0;
  while (members > 0) {
    w++;
    members >>= 1;
  }
  return w;
}

LCCOUNT_FN int counted_slots(int field_bits, int n_classes) {
  const int a = 64 - field_bits, b = 64 - n_classes;
  return a < b ? a : b;
}

LCCOUNT_FN int counted_fits(int n_classes, int slots) {
  return n_classes <= kCountedMaxClasses && slots >= 1;
}

}  // namespace lccount

#undef LCCOUNT_FN
