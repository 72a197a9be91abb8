"""Dev: lc_wr_check_lin (Elle's :linearizable-keys? inference on the device,
include/lincheck_wrlin.h) against lc_wr_check_lin_host, and against lc_wr_check
with the wfr inference alone (what a call costs without the inference), on one
GPU.  Not a test.

The history is wr.synth_arrays' (valid, shaped like the reference's :wr
workload).  The three calls alternate in one process: one warm-up of each, then
`reps` of each, every output compared between host and device each time;
median [min - max] of the library's own total_ms, kernel_ms, lin_kernel_ms and
host_graph_ms, and the touches, pairs, version edges and txn edges.  The
baseline is this project's own single-threaded host function, not Elle (none
is on these machines); no ratio is fixed in advance.
    python tools/wr_lin_probe.py [n_txns] [reps]
Prints one JSON line."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jepsen.etcd_amd import abi, wr as WR  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    n_txns = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    txns, mops = WR.synth_arrays(n_txns)
    ctx = abi.Context(device_mask=1)
    fields = ("total_ms", "kernel_ms", "host_graph_ms")
    laps = {who: {f: [] for f in fields} for who in ("lin_host", "lin_device", "wfr_device")}
    lin_kernel = []
    for rep in range(reps + 1):  # rep 0 warms all three up
        out_h, sh, lh = abi.wr_check_lin_host(txns, mops, True, True)
        out_d, sd, ld = ctx.wr_check_lin(txns, mops, True, True)
        _, sw = ctx.wr_check(txns, mops, True)
        assert all((out_d[f] == out_h[f]).all() for f in out_h), "device and host disagree"
        assert all(ld[f] == lh[f] for f in ld if f != "lin_kernel_ms"), "device and host disagree"
        if rep:
            for who, s in (("lin_host", sh), ("lin_device", sd), ("wfr_device", sw)):
                for f in fields:
                    laps[who][f].append(s[f])
            lin_kernel.append(ld["lin_kernel_ms"])
    ctx.close()
    print(json.dumps({
        "workload": "wr.synth_arrays(%d): %d mops, %d keys, %d versions" % (n_txns, len(mops), sd["n_keys"],
                                                                          sd["n_versions"]),
        "baseline": "lc_wr_check_lin_host, this project's own single-threaded host function (not Elle)",
        "valid": sd["valid"], "reps": reps, "touches": ld["n_touches"], "pairs": ld["n_pairs"],
        "version_edges": ld["n_vedges"], "max_key_versions": ld["max_key_versions"],
        "txn_edges": sd["n_edges"], "txn_edges_wfr_only": sw["n_edges"],
        "lin_host_ms": {f: spread(v) for f, v in laps["lin_host"].items()},
        "lin_device_ms": dict({f: spread(v) for f, v in laps["lin_device"].items()}, lin_kernel_ms=spread(lin_kernel)),
        "wfr_only_device_ms": {f: spread(v) for f, v in laps["wfr_device"].items()},
    }))


if __name__ == "__main__":
    main()
