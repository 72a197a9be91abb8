"""lc_set_full against lc_set_full_host at a ten-minute set run's size.

The history is built with numpy: `elements` adds by one process, `reads` reads
by `readers` processes, each read returning the set as it stood at a point
inside the read (defaults 50,000 x 4,000 by 5: about 10^8 payload entries).
The two functions alternate in one process after one warm-up each; the medians
of `runs` are printed with the device's copy / kernel / total split, then the
device alone with the payload page-locked (lc_host_register).  The
baseline is this project's single-threaded host function, the only CPU
implementation that exists here; it is not jepsen's.

With --profile the script then starts itself under `rocprofv3 --kernel-trace
--stats` (device calls only) and prints the per-kernel times.

    python tools/setfull_probe.py [--elements E] [--reads R] [--readers P] [--runs N]
                                  [--profile DIR]
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jepsen.etcd_amd import abi  # noqa: E402

RUN_NS = 600 * 10 ** 9  # a ten-minute run


def build(E, R, readers):
    """(adds, reads, values): every event has a place u in [0, 1); positions
    are the ranks of the places, times are u * RUN_NS."""
    per = -(-R // readers)
    a_inv = (np.arange(E) + 0.2) / E
    a_ok = (np.arange(E) + 0.8) / E
    j, k = np.arange(R) // readers, np.arange(R) % readers
    r_inv = (j + 0.1 + 0.02 * k) / per
    r_ok = (j + 0.9 + 0.02 * k) / per
    r_mid = (r_inv + r_ok) / 2
    u = np.concatenate([a_inv, a_ok, r_inv, r_ok])
    rank = np.empty(len(u), dtype=np.int64)
    rank[np.argsort(u, kind="stable")] = np.arange(len(u))
    t = (u * RUN_NS).astype(np.int64)
    adds = np.zeros(E, dtype=abi.SF_ADD_DTYPE)
    adds["value"] = np.arange(E)
    adds["inv_pos"], adds["ok_pos"], adds["ok_time"] = rank[:E], rank[E:2 * E], t[E:2 * E]
    order = np.argsort(rank[2 * E + R:])  # reads in ok_pos order
    reads = np.zeros(R, dtype=abi.SF_READ_DTYPE)
    reads["inv_pos"], reads["ok_pos"] = rank[2 * E:2 * E + R][order], rank[2 * E + R:][order]
    reads["inv_time"], reads["ok_time"] = t[2 * E:2 * E + R][order], t[2 * E + R:][order]
    seen = np.searchsorted(a_ok, r_mid[order])  # the acknowledged adds at the read's point
    reads["len"] = seen
    reads["off"] = np.cumsum(seen) - seen
    values = np.concatenate([np.arange(m, dtype=np.int64) for m in seen]) if R else np.zeros(0, np.int64)
    return adds, reads, values


def kernel_stats(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    return [{"kernel": re.search(r"sf_\w+", r["Name"]).group(0), "calls": int(r["Calls"]),
             "total_ms": float(r["TotalDurationNs"]) / 1e6, "avg_ms": float(r["AverageNs"]) / 1e6}
            for r in rows if "sf_" in r["Name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=50000)
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--readers", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--device-only", action="store_true", help="(the profiled child)")
    a = ap.parse_args()
    t0 = time.perf_counter()
    adds, reads, values = build(a.elements, a.reads, a.readers)
    print(json.dumps({"probe": "setfull", "elements": a.elements, "reads": a.reads, "readers": a.readers,
                      "payload_entries": int(len(values)), "build_s": round(time.perf_counter() - t0, 2)}),
          flush=True)
    with abi.Context(device_mask=1) as ctx:
        dev, host, want = [], [], None
        for i in range(a.runs + 1):  # the first of each is the warm-up
            got, s = ctx.set_full(adds, reads, values)
            dev.append(s)
            if not a.device_only:
                want, hs = abi.set_full_host(adds, reads, values)
                host.append(hs)
                if (want != got).any():
                    raise SystemExit("device and host disagree")
        # the payload page-locked (lc_host_register), as a caller that keeps its buffer would
        pinned = []
        if not a.device_only:
            ctx.host_register(values)
            for i in range(a.runs + 1):
                pinned.append(ctx.set_full(adds, reads, values)[1])
            ctx.host_unregister(values)
    med = lambda xs: round(statistics.median(xs), 3)  # noqa: E731
    out = {"device_total_ms": med([s["total_ms"] for s in dev[1:]]),
           "device_h2d_ms": med([s["h2d_ms"] for s in dev[1:]]),
           "device_kernel_ms": med([s["kernel_ms"] for s in dev[1:]]),
           "device_total_ms_runs": [round(s["total_ms"], 3) for s in dev[1:]],
           "n_tiles": dev[-1]["n_tiles"], "valid": dev[-1]["valid"],
           "counts": {k: dev[-1][k] for k in ("n_stable", "n_lost", "n_never_read", "n_stale", "n_phantom")}}
    if host:
        out["device_pinned_total_ms"] = med([s["total_ms"] for s in pinned[1:]])
        out["device_pinned_h2d_ms"] = med([s["h2d_ms"] for s in pinned[1:]])
        out["host_total_ms"] = med([s["total_ms"] for s in host[1:]])
        out["host_total_ms_runs"] = [round(s["total_ms"], 3) for s in host[1:]]
        out["host_over_device"] = round(out["host_total_ms"] / out["device_total_ms"], 2)
        out["baseline"] = "lc_set_full_host (this project's single-threaded host function, not jepsen)"
    print(json.dumps(out), flush=True)
    if a.profile:
        os.makedirs(a.profile, exist_ok=True)
        # a fresh child under the profiler: device calls only
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", a.profile, "-o", "kt",
                               "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                               "--elements", str(a.elements), "--reads", str(a.reads), "--readers",
                               str(a.readers), "--runs", "2", "--device-only"],
                              stdout=subprocess.DEVNULL)
        for r in kernel_stats(a.profile):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
