"""Dev: lc_append_check (graph on the device) against lc_append_check_host, on
one GPU.  Not a test.

The history is built with numpy alone (append.synth_arrays): valid, about
10^6 txns shaped like the reference's :append workload — 3 live keys, up to 4
mops per txn, 32 appends per key before it is retired, concurrency 10, 3 %
INFO.  The two calls alternate in one process: one warm-up of each, then 5 of
each; medians and ranges.  The baseline is this project's own host function,
not Elle (none is on these machines), and no ratio is fixed in advance.
host_graph_ms (rule 7 on the host) against kernel_ms says whether a device
SCC search is worth building next.
    python tools/append_probe.py [n_txns] [reps]
Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jepsen.etcd_amd import abi, append as AP  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    n_txns = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    txns, mops, values = AP.synth_arrays(n_txns, seed=1)
    ctx = abi.Context(device_mask=1)
    laps = {"device": [], "host": []}
    parts = {k: [] for k in ("h2d_ms", "kernel_ms", "host_graph_ms", "total_ms")}
    host_parts = {k: [] for k in ("host_graph_ms", "total_ms")}
    summary = None
    for rep in range(reps + 1):  # rep 0 warms both up
        t0 = time.perf_counter()
        out_d, sd = ctx.append_check(txns, mops, values)
        t1 = time.perf_counter()
        out_h, sh = abi.append_check_host(txns, mops, values)
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
        "workload": "valid list-append history, numpy-built: %d txns, %d mops, %d payload entries referenced, "
                    "%d keys, %d edges" % (n_txns, len(mops), int(mops["len"][mops["len"] > 0].sum()),
                                           summary["n_keys"], summary["n_edges"]),
        "baseline": "lc_append_check_host, this project's own single-threaded host function (not Elle)",
        "valid": summary["valid"], "n_slow_reads": summary["n_slow_reads"], "reps": reps,
        "device_call_ms": spread(laps["device"]), "host_call_ms": spread(laps["host"]),
        "device_parts_ms": {k: spread(v) for k, v in parts.items()},
        "host_parts_ms": {k: spread(v) for k, v in host_parts.items()},
        "host_graph_over_kernel": round(statistics.median(parts["host_graph_ms"]) /
                                        max(statistics.median(parts["kernel_ms"]), 1e-9), 2),
    }))


if __name__ == "__main__":
    main()
