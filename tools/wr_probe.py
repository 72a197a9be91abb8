"""Dev: lc_wr_check (version graphs and dependency graph on the device) against
lc_wr_check_host, on one GPU.  Not a test.

The history is built with numpy alone (wr.synth_arrays): valid, about 10^6
txns shaped like the reference's :wr workload — 3 live keys, up to 4 mops per
txn, 32 writes per key before it is retired, concurrency 10, 3 % INFO.  The
two calls alternate in one process: one warm-up of each, then 5 of each;
medians and ranges of the library's own total_ms, split into the copy, the
kernels and the host's rule 9.  The baseline is this project's own host
function, not Elle (none is on these machines), and no ratio is fixed in
advance.  host_graph_ms against kernel_ms says whether a device SCC search is
the follow-up for both Elle checkers.
    python tools/wr_probe.py [n_txns] [reps] [wfr: 1 | 0]
Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jepsen.etcd_amd import abi, wr as WR  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    n_txns = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    wfr = bool(int(sys.argv[3])) if len(sys.argv) > 3 else True
    txns, mops = WR.synth_arrays(n_txns, seed=1)
    ctx = abi.Context(device_mask=1)
    laps = {"device": [], "host": []}
    parts = {k: [] for k in ("h2d_ms", "kernel_ms", "host_graph_ms", "total_ms")}
    host_parts = {k: [] for k in ("host_graph_ms", "total_ms")}
    summary = None
    for rep in range(reps + 1):  # rep 0 warms both up
        t0 = time.perf_counter()
        out_d, sd = ctx.wr_check(txns, mops, wfr)
        t1 = time.perf_counter()
        out_h, sh = abi.wr_check_host(txns, mops, wfr)
        t2 = time.perf_counter()
        assert all((out_d[f] == out_h[f]).all() for f in out_h), "device and host disagree"
        if rep:
            laps["device"].append((t1 - t0) * 1e3)
            laps["host"].append((t2 - t1) * 1e3)
            for k in parts:
                parts[k].append(sd[k])
            for k in host_parts:
                host_parts[k].append(sh[k])
        summary = sd
    ctx.close()
    print(json.dumps({
        "workload": "valid rw-register history, numpy-built: %d txns, %d mops, %d keys, %d versions, %d edges "
                    "(%d before unique), wfr %s" % (n_txns, len(mops), summary["n_keys"], summary["n_versions"],
                                                    summary["n_edges"], summary["n_edges_raw"], wfr),
        "baseline": "lc_wr_check_host, this project's own single-threaded host function (not Elle)",
        "valid": summary["valid"], "reps": reps,
        "device_call_ms": spread(laps["device"]), "host_call_ms": spread(laps["host"]),
        "device_parts_ms": {k: spread(v) for k, v in parts.items()},
        "host_parts_ms": {k: spread(v) for k, v in host_parts.items()},
        "host_graph_over_kernel": round(statistics.median(parts["host_graph_ms"]) /
                                        max(statistics.median(parts["kernel_ms"]), 1e-9), 2),
    }))


if __name__ == "__main__":
    main()
