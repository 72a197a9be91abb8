// cert_layout.h — the PROOF search's scratch inside one key's workspace
// (cert.hip, cert_kernel).  Host code may include this: plain constexpr.
//
// By the time wave 0 searches for a PROOF the key's lower-bound array (lo64:
// n + 2 uint64, that is 2 (n + 2) int32) is free.  It is carved into the log
// of assumed positions and the stack of open case splits:
//   logp    cert_logp_ints(n) int32: one per assumed position; the open
//           positions number at most the mutations of the key, so n suffice;
//   frames  cert_n_frames(n) frames of kCertFrameInts int32 each — the ints
//           left after logp.
// The frames are plain int32 fields: the region starts at an int32 offset of
// 2 (records before the key + 2 keys before it), which is only 8-byte
// aligned when that count is odd, so no wider access is made to it.
#pragma once

namespace lcdev {

constexpr int kCertFrameInts = 4;  // position, cases << 16 | case, log length, op assumed

constexpr int cert_key_ints(int n) { return 2 * (n + 2); }
constexpr int cert_logp_ints(int n) { return n + 2; }
constexpr int cert_n_frames(int n) {
  return (cert_key_ints(n) - cert_logp_ints(n)) / kCertFrameInts;
}

// logp plus frames stay inside the key's own 2 (n + 2) ints, and logp holds
// one entry per possible open position, for every key size
constexpr bool cert_layout_fits(int n_max) {
  for (int n = 0; n <= n_max; n++) {
    if (cert_logp_ints(n) < n) return false;
    if (cert_n_frames(n) < 0) return false;
    if (cert_logp_ints(n) + kCertFrameInts * cert_n_frames(n) > cert_key_ints(n)) return false;
  }
  return true;
}
static_assert(cert_layout_fits(4096), "PROOF scratch overruns the key's lo64 region");

}  // namespace lcdev
