// Dev, run by hand on a CPU machine: lc_append_check_host under
// AddressSanitizer and UBSan, as a stand-alone program (host code only; no
// GPU, no python).  From the repository's root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/append_host_sanitize.cpp jepsen/etcd_amd/csrc/append_host.cpp \
//       jepsen/etcd_amd/csrc/graph_host.cpp -o /tmp/append_host_sanitize
//   /tmp/append_host_sanitize
// It runs a few of tests/golden/append_kat.json's histories, written out
// below as arrays, a refused input, and an SCC with every edge type; prints
// one line per case and exits non-zero on a wrong verdict.
#include <stdio.h>

#include <vector>

#include "../include/lincheck_append.h"

namespace {

struct Case {
  const char *name;
  std::vector<lc_ap_txn> txns;
  std::vector<lc_ap_mop> mops;
  std::vector<int64_t> values;
  int want_rc, want_valid;
};

lc_ap_mop A(int64_t k, int64_t e) { return lc_ap_mop{k, e, LC_AP_APPEND, 0}; }
lc_ap_mop R(int64_t k, int64_t off, int32_t len) { return lc_ap_mop{k, off, LC_AP_READ, len}; }
lc_ap_txn T(int64_t off, int32_t inv, int32_t comp, int32_t type, int32_t len) {
  return lc_ap_txn{off, inv, comp, type, len};
}

int run(const Case &c) {
  const size_t nt = c.txns.size(), nm = c.mops.size();
  std::vector<int32_t> mop_flags(nm + 1), txn_flags(nt + 1), byc(nt + 1), lo(nt + 1), hi(nt + 1), scc(nt + 1),
      cls(nt + 1), cycle_scc(LC_AP_MAX_CYCLES);
  std::vector<lc_ap_key> keys(nm + 1);
  std::vector<lc_ap_edge> edges(2 * nm + 1);
  std::vector<lc_ap_step> steps(nt + 1);
  std::vector<int64_t> cycle_off(LC_AP_MAX_CYCLES + 1);
  lc_ap_out out{mop_flags.data(), txn_flags.data(), keys.data(), edges.data(), byc.data(), lo.data(),
                hi.data(),        scc.data(),       cls.data(),  steps.data(), cycle_off.data(), cycle_scc.data()};
  lc_ap_summary s{};
  const int rc = lc_append_check_host(c.txns.data(), (int64_t)nt, c.mops.data(), (int64_t)nm, c.values.data(),
                                      (int64_t)c.values.size(), &out, &s);
  const bool ok = rc == c.want_rc && (rc != 0 || s.valid == c.want_valid);
  printf("%-22s rc %d valid %d edges %lld sccs %lld cycles %lld %s\n", c.name, rc, rc ? 0 : s.valid,
         (long long)s.n_edges, (long long)s.n_scc, (long long)s.n_cycles_returned, ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}

}  // namespace

int main() {
  std::vector<Case> cases;
  // "valid": T0 appends 1; T1 reads [1], appends 2; T2 reads [1 2]
  cases.push_back({"valid",
                   {T(0, 0, 1, LC_AP_OK, 1), T(1, 2, 3, LC_AP_OK, 2), T(3, 4, 5, LC_AP_OK, 1)},
                   {A(1, 1), R(1, 0, 1), A(1, 2), R(1, 1, 2)},
                   {1, 1, 2}, 0, 1});
  // "G0": concurrent T0, T1 append to keys 1 and 2; T2 reads [1 3] and [4 2]
  cases.push_back({"G0",
                   {T(0, 0, 2, LC_AP_OK, 2), T(2, 1, 3, LC_AP_OK, 2), T(4, 4, 5, LC_AP_OK, 2)},
                   {A(1, 1), A(2, 2), A(1, 3), A(2, 4), R(1, 0, 2), R(2, 2, 2)},
                   {1, 3, 4, 2}, 0, 0});
  // "G2-item-realtime" of the fixture: rw, rt, rw, wr
  cases.push_back({"G2-item-realtime",
                   {T(0, 0, 7, LC_AP_OK, 2), T(2, 1, 6, LC_AP_OK, 1), T(3, 2, 3, LC_AP_OK, 1),
                    T(4, 4, 5, LC_AP_OK, 1), T(5, 8, 9, LC_AP_OK, 2)},
                   {R(1, 0, 0), R(2, 0, 1), A(2, 2), A(1, 1), R(2, 0, 0), R(1, 1, 1), R(2, 0, 1)},
                   {2, 1}, 0, 0});
  // non-prefix read with a duplicate and a failed element; an internal read; a phantom
  cases.push_back({"anomalies",
                   {T(0, 0, 1, LC_AP_OK, 1), T(1, 2, 3, LC_AP_FAIL, 1), T(2, 4, 5, LC_AP_OK, 1),
                    T(3, 6, 7, LC_AP_OK, 3), T(6, 8, -1, LC_AP_INFO, 2)},
                   {A(1, 1), A(1, 2), R(1, 0, 3), R(1, 3, 3), A(1, 5), R(1, 0, 1), A(1, 6), R(1, 0, -1)},
                   {1, 2, 9, 2, 2, 1}, 0, 0});
  // two appends of one (key, element): refused
  cases.push_back({"pair-twice", {T(0, 0, 1, LC_AP_OK, 2)}, {A(1, 1), A(1, 1)}, {}, -22, 0});
  // no OK txn: unknown
  cases.push_back({"no-ok-txn", {T(0, 0, -1, LC_AP_INFO, 1)}, {A(1, 1)}, {}, 0, -1});
  int bad = 0;
  for (const Case &c : cases) bad += run(c);
  return bad ? 1 : 0;
}
