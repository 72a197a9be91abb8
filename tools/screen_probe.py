"""Dev: the screened checker calls (lc_append_check_screened,
lc_wr_check_screened: the cycle screen run on the device, the host graph pass
skipped where it proves the graph clean) against the unscreened ones, on one
GPU.  Not a test.

The histories are the two Elle probes' own (append.synth_arrays and
wr.synth_arrays, about 10^6 txns, valid), and each of them again with one
stale read planted near its end, which makes it invalid with one SCC of about
5,000 txns (the host pass takes minutes on an SCC of 10^5):
what an invalid history pays for a screen that cannot skip.  Per history the
screened and the unscreened call alternate in one process: one warm-up of
each, then `reps` of each; median [min-max] of the library's own numbers, and
every output array and count compared.
    python tools/screen_probe.py [n_txns] [reps]
Prints one JSON line per history."""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jepsen.etcd_amd import abi, append as AP, wr as WR  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def _late_read(txns, mops, is_read):
    """The last read by an OK txn among the last 1,000 txns that is alone in its txn."""
    for t in range(len(txns) - 1, max(len(txns) - 1000, 0) - 1, -1):
        m = int(txns["mop_off"][t])
        if txns["type"][t] == abi.LC_AP_OK and txns["mop_len"][t] == 1 and is_read(m):
            return m
    raise RuntimeError("no read to make stale")


BACK = 5000  # how many txns back the planted read looks: the SCC holds about that many


def stale_append(txns, mops, values):
    """A read near the end answers as a non-empty read BACK txns before it did:
    a prefix of a key that has grown since."""
    mops = mops.copy()
    first = int(txns["mop_off"][max(len(txns) - BACK, 0)])
    early = first + int(np.nonzero((mops["f"][first:] == abi.LC_AP_READ) & (mops["len"][first:] >= 1))[0][0])
    m = _late_read(txns, mops, lambda m: mops["f"][m] == abi.LC_AP_READ and mops["len"][m] >= 0)
    mops[m] = mops[early]
    return txns, mops, values


def stale_wr(txns, mops):
    """A read near the end answers with a value that a txn BACK txns before it
    read and overwrote."""
    mops = mops.copy()
    m = _late_read(txns, mops, lambda m: mops["f"][m] == abi.LC_WR_READ and mops["known"][m] == 1)
    for t in range(max(len(txns) - BACK, 0), len(txns)):
        lo, hi = int(txns["mop_off"][t]), int(txns["mop_off"][t]) + int(txns["mop_len"][t])
        for i in range(lo, hi):
            if txns["type"][t] == abi.LC_WR_OK and mops["f"][i] == abi.LC_WR_READ and mops["known"][i] and \
                    mops["value"][i] != abi.LC_WR_NIL and not (mops["key"][lo:i] == mops["key"][i]).any() and \
                    ((mops["key"][i + 1:hi] == mops["key"][i]) & (mops["f"][i + 1:hi] == abi.LC_WR_WRITE)).any():
                mops["key"][m], mops["value"][m] = mops["key"][i], mops["value"][i]
                return txns, mops
    raise RuntimeError("no overwritten read to repeat")


COUNTS = ("valid", "n_class", "n_keys", "n_ok", "n_nodes", "n_edges", "n_scc", "n_cycles_returned")


def probe(name, plain, screened, reps):
    rows = {k: [] for k in ("total_ms", "host_graph_ms", "kernel_ms", "screened_total_ms", "screened_host_graph_ms",
                            "screened_kernel_ms", "screen_kernel_ms", "screen_total_ms")}
    for rep in range(reps + 1):  # rep 0 warms both up
        out, s = plain()
        out2, s2, sc = screened()
        if rep:
            for k, v in (("total_ms", s["total_ms"]), ("host_graph_ms", s["host_graph_ms"]),
                         ("kernel_ms", s["kernel_ms"]), ("screened_total_ms", s2["total_ms"]),
                         ("screened_host_graph_ms", s2["host_graph_ms"]), ("screened_kernel_ms", s2["kernel_ms"]),
                         ("screen_kernel_ms", sc["kernel_ms"]), ("screen_total_ms", sc["total_ms"])):
                rows[k].append(v)
    assert all((out[f] == out2[f]).all() for f in out) and all(s[k] == s2[k] for k in COUNTS), "the calls disagree"
    assert (sc["clean"] == 1) == (s["n_scc"] == 0), (sc, s["n_scc"])
    print(json.dumps({"history": name, "n_txns": len(out["txn_flags"]), "n_edges": s["n_edges"], "valid": s["valid"],
                      "n_scc": s["n_scc"], "scc_members": int((out["scc"] >= 0).sum()), "clean": sc["clean"],
                      "label_rounds": sc["label_rounds"], "trim_rounds": sc["trim_rounds"],
                      "max_rounds": sc["max_rounds"], "n_rt_members": sc["n_rt_members"],
                      "n_trim_survivors": sc["n_trim_survivors"], "reps": reps,
                      **{k: spread(v) for k, v in rows.items()}}), flush=True)


def main():
    n_txns = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = abi.Context(device_mask=1)
    ap = AP.synth_arrays(n_txns, seed=1)
    probe("append valid", lambda: ctx.append_check(*ap), lambda: ctx.append_check_screened(*ap), reps)
    bad = stale_append(*ap)
    probe("append stale-read", lambda: ctx.append_check(*bad), lambda: ctx.append_check_screened(*bad), reps)
    del ap, bad
    wr = WR.synth_arrays(n_txns, seed=1)
    probe("wr valid", lambda: ctx.wr_check(*wr), lambda: ctx.wr_check_screened(*wr), reps)
    bad = stale_wr(*wr)
    probe("wr stale-read", lambda: ctx.wr_check(*bad), lambda: ctx.wr_check_screened(*bad), reps)
    ctx.close()


if __name__ == "__main__":
    main()
