"""Dev: lc_watch_check (log hashes, exact compares, Myers' forward pass and the
backtrack on the device) against lc_watch_check_host, on one GPU.  Not a test.

The logs are built with numpy (watch.synth_arrays): n_threads threads of one
random log of n_values events.  Two cases: every log equal (the valid case:
hashes and one compare per thread, memory bound), and a few threads with a few
scattered edits (the invalid case: long snakes between the edits).  The two
calls alternate in one process: one warm-up of each, then `reps` of each;
medians and ranges of the library's own total_ms, h2d_ms and kernel_ms.  The
baseline is this project's own single-threaded host function — the only CPU
implementation there is; it is not jepsen — and no ratio is fixed in advance.
    python tools/watch_probe.py [n_threads] [n_values] [reps]
Prints one JSON line per case."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jepsen.etcd_amd import abi, watch as W  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def case(ctx, name, threads, values, reps):
    dev = {k: [] for k in ("total_ms", "h2d_ms", "kernel_ms")}
    host = []
    summary = None
    for rep in range(reps + 1):  # rep 0 warms both up
        out_d, sd = ctx.watch_check(threads, values)
        out_h, sh = abi.watch_check_host(threads, values)
        assert all((out_d[f] == out_h[f]).all() for f in out_h), "device and host disagree"
        if rep:
            for k in dev:
                dev[k].append(sd[k])
            host.append(sh["total_ms"])
        summary = sd
    print(json.dumps({
        "case": name,
        "workload": "%d threads x %d values (%.0f MB), %d classes, %d deltas, %d edits, largest distance %d"
                    % (len(threads), int(threads["len"][0]), values.nbytes / 1e6, summary["n_classes"],
                       summary["n_deltas"], summary["n_edits"], int(out_d["distance"].max())),
        "baseline": "lc_watch_check_host, this project's own single-threaded host function (not jepsen)",
        "valid": summary["valid"], "reps": reps,
        "device_ms": {k: spread(v) for k, v in dev.items()},
        "host_total_ms": spread(host),
        "host_over_device": round(statistics.median(host) / max(statistics.median(dev["total_ms"]), 1e-9), 2),
    }), flush=True)


def main():
    n_threads = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    n_values = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    ctx = abi.Context(device_mask=1)
    case(ctx, "all logs equal", *W.synth_arrays(n_threads, n_values, None, seed=1), reps)
    edits = {n_threads // 6: 3, n_threads // 2: 2, n_threads - 3: 4} if n_threads >= 6 else {n_threads - 1: 3}
    case(ctx, "threads %s with %s scattered edits" % (sorted(edits), [edits[t] for t in sorted(edits)]),
         *W.synth_arrays(n_threads, n_values, edits, seed=1), reps)
    ctx.close()


if __name__ == "__main__":
    main()
