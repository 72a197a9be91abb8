"""Dev: the restricted checker calls (lc_append_check_restricted,
lc_wr_check_restricted: the host graph pass over the screen's marked txns, the
txn that closes a G-single cycle searched on the device) against the screened
and the unscreened ones, and lc_cycle_reach against lc_cycle_reach_host, on one
GPU.  Not a test.

The histories are tools/screen_probe.py's: the two Elle probes' own valid ones
of about 10^6 txns, and each again with one stale read planted near its end
that looks BACK txns back, for BACK = 5,000 and, where the unscreened call
finishes within LIMIT_S seconds, 50,000 (otherwise the probe halves BACK until
it does, and says which it took).  Per history the three calls alternate in
one process: one warm-up of each, then `reps` of each; median [min-max] of the
library's own numbers, and every output array and count compared.

Then the stand-alone primitive on the component each stale-read history
produces (the hook's own problem, recorded through lc_cycles_host), and on
synthetic components (a chain with a skip edge every 8 nodes, every node a
candidate whose head does not reach it: the worst case, every search runs to
the end) sweeping candidates x (nodes + preds): the least work at which the
device call is faster than the host loop is the crossover default_min_work is
derived from.
    python tools/cycle_search_probe.py [n_txns] [reps] [BACKs, comma-separated; "-": the sweep alone]
Prints one JSON line per history, per component and per sweep point."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import screen_probe as SP  # noqa: E402
from jepsen.etcd_amd import abi, append as AP, wr as WR  # noqa: E402

LIMIT_S = 120.0
COUNTS = SP.COUNTS


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def probe(name, plain, screened, restricted, reps):
    keys = ("total_ms", "host_graph_ms")
    rows = {"%s_%s" % (c, k): [] for c in ("unscreened", "screened", "restricted") for k in keys}
    rows["search_ms"] = []
    for rep in range(reps + 1):  # rep 0 warms all three up
        out, s = plain()
        out2, s2, sc2 = screened()
        out3, s3, sc3, srch = restricted()
        if rep:
            for c, x in (("unscreened", s), ("screened", s2), ("restricted", s3)):
                for k in keys:
                    rows["%s_%s" % (c, k)].append(x[k])
            rows["search_ms"].append(srch["search_ms"])
    for o, x in ((out2, s2), (out3, s3)):
        assert all((out[f] == o[f]).all() for f in out) and all(s[k] == x[k] for k in COUNTS), "the calls disagree"
    below = max(rows["restricted_host_graph_ms"]) < min(rows["screened_host_graph_ms"])
    print(json.dumps({"history": name, "n_txns": len(out["txn_flags"]), "n_edges": s["n_edges"], "valid": s["valid"],
                      "n_scc": s["n_scc"], "scc_members": int((out["scc"] >= 0).sum()), "clean": sc3["clean"],
                      "restricted": srch["restricted"], "n_marked": srch["n_marked"],
                      "n_device_searches": srch["n_device_searches"], "n_device_queries": srch["n_device_queries"],
                      "n_host_fallbacks": srch["n_host_fallbacks"], "reps": reps,
                      "every_restricted_host_graph_ms_below_every_screened": bool(below),
                      **{k: spread(v) for k, v in rows.items()}}), flush=True)
    return out, s


def component(ctx, name, txns, out, reps):
    """The G-single search of the history's SCC as the hook receives it, on the device and on the host."""
    arrays, _ = abi.cycle_screen_host(txns, out["edges"])
    seen = []

    def record(n, po, pr, qn, qo, qh):
        seen.append((int(n), po.copy(), pr.copy(), qn.copy(), qo.copy(), qh.copy()))
        return abi.cycle_reach_host(n, po, pr, qn, qo, qh)[1]["first_hit"]

    abi.cycles_host(txns, out["edges"], arrays["mark"], record, min_work=0)
    for args in seen:
        reach(ctx, name, args, reps)


def reach(ctx, name, args, reps):
    dev, host, kern = [], [], []
    for rep in range(reps + 1):
        _, d = ctx.cycle_reach(*args)
        _, h = abi.cycle_reach_host(*args)
        assert d["first_hit"] == h["first_hit"], (d, h)
        if rep:
            dev.append(d["total_ms"])
            kern.append(d["kernel_ms"])
            host.append(h["total_ms"])
    n, po, pr, qn = args[0], args[1], args[2], args[3]
    print(json.dumps({"reach": name, "n_nodes": n, "n_pred": len(pr), "n_queries": len(qn),
                      "work": len(qn) * (n + len(pr)), "first_hit": d["first_hit"], "device_total_ms": spread(dev),
                      "device_kernel_ms": spread(kern), "host_total_ms": spread(host),
                      "device_faster": statistics.median(dev) < statistics.median(host)}), flush=True)


def synthetic(n, n_queries):
    """i + 1 -> i and i + 8 -> i; the first n_queries nodes ask for node 0's successor side: a head below them."""
    frm = np.concatenate([np.arange(1, n), np.arange(8, n)])
    to = np.concatenate([np.arange(0, n - 1), np.arange(0, n - 8)])
    order = np.argsort(to, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(to, minlength=n), out=off[1:])
    qn = np.arange(1, min(n_queries, n - 1) + 1, dtype=np.int32)
    n_queries = len(qn)
    return n, off, frm[order].astype(np.int32), qn, np.arange(n_queries + 1, dtype=np.int64), (qn - 1).astype(np.int32)


def stale(ctx, kind, base, plant, back, reps):
    """The three calls on `base` with a read planted that looks `back` txns back (halved until the unscreened call fits)."""
    while True:
        SP.BACK = back
        bad = plant(*base)
        call = ctx.append_check if kind == "append" else ctx.wr_check
        t0 = time.time()
        call(*bad)
        if time.time() - t0 <= LIMIT_S or back <= 5000:
            break
        print(json.dumps({"history": "%s stale-read" % kind, "back": back, "skipped": "unscreened call above %gs" % LIMIT_S}),
              flush=True)
        back //= 2
    if kind == "append":
        out, _ = probe("append stale-read back=%d" % back, lambda: ctx.append_check(*bad),
                       lambda: ctx.append_check_screened(*bad), lambda: ctx.append_check_restricted(*bad), reps)
    else:
        out, _ = probe("wr stale-read back=%d" % back, lambda: ctx.wr_check(*bad), lambda: ctx.wr_check_screened(*bad),
                       lambda: ctx.wr_check_restricted(*bad), reps)
    component(ctx, "%s back=%d" % (kind, back), bad[0], out, reps)


def main():
    n_txns = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    backs = [5000, 50000] if len(sys.argv) <= 3 else [int(b) for b in sys.argv[3].split(",") if b != "-"]
    print(json.dumps({"limits": abi.cycle_reach_limits()}), flush=True)
    ctx = abi.Context(device_mask=1)
    if backs:
        ap = AP.synth_arrays(n_txns, seed=1)
        probe("append valid", lambda: ctx.append_check(*ap), lambda: ctx.append_check_screened(*ap),
              lambda: ctx.append_check_restricted(*ap), reps)
        for back in backs:
            stale(ctx, "append", ap, SP.stale_append, back, reps)
        del ap
        wr = WR.synth_arrays(n_txns, seed=1)
        probe("wr valid", lambda: ctx.wr_check(*wr), lambda: ctx.wr_check_screened(*wr),
              lambda: ctx.wr_check_restricted(*wr), reps)
        for back in backs:
            stale(ctx, "wr", wr, SP.stale_wr, back, reps)
        del wr
    for n, q in ((64, 8), (64, 64), (256, 8), (256, 32), (256, 256), (1024, 8), (1024, 32), (1024, 64), (1024, 256),
                 (1024, 1024), (4096, 8), (4096, 32), (4096, 256), (4096, 1024), (4096, 4096), (16384, 8), (16384, 64),
                 (16384, 1024), (16384, 4096)):
        reach(ctx, "synthetic", synthetic(n, q), reps)
    ctx.close()


if __name__ == "__main__":
    main()
