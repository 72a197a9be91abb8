"""Dev: lc_check_events (split and completion on the device) against the host
preparation it replaces, on one GPU.

Default workload: the history of tools/edn_e2e.py (1,000 keys x 1,000 ops,
concurrency 20, 2 % crashed ops, seed 5, ~2.5 M events).  Baseline: the
native reader's `split` + `complete` + `gather` laps (LC_EDN_TIMING, 16
threads) plus its lc_check16 call.  New: lc_check_events' wall time with the
lc_last_events_stats breakdown.  The two alternate in one process: one
warm-up of each, then 5 of each; medians and ranges.  The event encoding is
not timed (a binding writes events where it writes op maps today).
    python tools/events_probe.py [keys] [ops_per_key] [threads] [reps]
    python tools/events_probe.py --synth [keys] [ops_per_key] [reps]
--synth: the events built directly with numpy from abi.synth_key streams (no
op maps, no EDN), e.g. 10000 1000 for C2's size; the comparison is then
lc_check32 on the host-packed records.
Prints one JSON line."""
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jepsen.etcd_amd import abi, edn, events as E, synth  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


class Stderr:
    """The process's stderr (fd 2, where the native reader prints its laps)
    into a file for the length of a with block."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def laps(text):
    return {m.group(1): float(m.group(2)) for m in re.finditer(r"lc_edn (\w+)\s+([\d.]+) ms", text)}


def new_path(ctx, ev, n_keys, opts):
    a = time.perf_counter()
    _, res = ctx.check_events(ev, n_keys, opts)
    wall = (time.perf_counter() - a) * 1e3
    return wall, ctx.last_events_stats(), res


def synth_events(nk, n):
    """The events of nk keys of abi.synth_key, interleaved by local time."""
    parts = []
    for k in range(nk):
        ops, proc, st, _ = abi.synth_key(k, n, 20, 5, 0.02, 0.0, 5)
        m = len(ops)
        f, v, e, ver, call, ret = (ops[:, i] for i in range(6))
        inv = np.zeros((m, 6), dtype=np.int64)
        inv[:, 0], inv[:, 1], inv[:, 2] = k, k * 100000 + proc, f << 8
        inv[:, 3] = np.where(f == abi.LC_F_READ, -1, v)
        inv[:, 4] = np.where(f == abi.LC_F_CAS, e, -1)
        inv[:, 5] = -1
        comp = inv.copy()
        comp[:, 2] |= np.where(st == 1, E.LC_EV_OK, np.where(st == 0, E.LC_EV_FAIL, E.LC_EV_INFO))
        ok = st == 1
        comp[ok, 3], comp[ok, 5] = v[ok], ver[ok]
        done = st != 2
        last = int(max(call.max(), ret[done].max() if done.any() else 0))
        when = np.where(done, ret, last + 1 + np.cumsum(~done))
        t = np.concatenate([call, when])
        parts.append((t, np.full(2 * m, k), np.concatenate([np.zeros(m, int), np.ones(m, int)]),
                      np.concatenate([inv, comp])))
    t, key, order, rows = (np.concatenate([p[i] for p in parts]) for i in range(4))
    return rows[np.lexsort((order, key, t))].astype(np.int32)


def main(argv):
    if argv and argv[0] == "--synth":
        nk, n, reps = (int(x) for x in (argv[1:] + ["10000", "1000", "5"][len(argv) - 1:]))
        ev = synth_events(nk, n)
        host = abi.pack_events_host(ev, nk)
        out = {"workload": "synth", "keys": nk, "ops_per_key": n, "events": len(ev), "records": len(host[0])}
        opts = abi.default_opts()
        old, new, parts = [], [], []
        with abi.Context(device_mask=1) as ctx:
            for rep in range(reps + 1):
                a = time.perf_counter()
                _, ref = ctx.check32(host[0], host[1], host[2], opts)
                b = (time.perf_counter() - a) * 1e3
                wall, st, res = new_path(ctx, ev, nk, opts)
                assert (res == ref).all()
                if rep:
                    old.append(b)
                    new.append(wall)
                    parts.append(st)
        out["check32_on_host_pack_ms"] = spread(old)
    else:
        nk, n, threads, reps = (int(x) for x in (argv + ["1000", "1000", "16", "5"][len(argv):]))
        hist, _ = synth.jepsen_history(nk, n, concurrency=20, p_info=0.02, seed=5)
        path = os.path.join(tempfile.gettempdir(), "lc_events_probe.edn")
        with open(path, "w") as f:
            f.write(edn.to_edn(hist))
        ev, keys, _, _ = E.encode(hist)
        del hist
        out = {"workload": "edn_e2e", "keys": nk, "ops_per_key": n, "threads": threads,
               "events": len(ev)}
        opts = abi.default_opts(flags=abi.LC_FLAG_WHOLE_GPU)  # edn.check's options
        os.environ["LC_EDN_TIMING"] = "1"
        old, new, parts, prep, chk = [], [], [], [], []
        with abi.Context(device_mask=1) as ctx:
            for rep in range(reps + 1):
                with Stderr() as err:
                    h = edn.read(path, n_threads=threads)
                lp = laps(err.text)
                o16, base = h.ops16()
                a = time.perf_counter()
                _, ref = ctx.check16(o16, h.key_off, base, opts=opts)
                c16 = (time.perf_counter() - a) * 1e3
                wall, st, res = new_path(ctx, ev, len(keys), opts)
                mine = {str(k): (int(r["verdict"]), int(r["fail_op"])) for k, r in zip(keys, res)}
                theirs = {k: (int(r["verdict"]), int(r["fail_op"])) for k, r in zip(h.keys, ref)}
                assert mine == theirs
                out["records"] = int(h.key_off[-1])
                assert out["records"] == st["n_ops"]
                del h
                if rep:
                    p = lp["split"] + lp["complete"] + lp["gather"]
                    prep.append(p)
                    chk.append(c16)
                    old.append(p + c16)
                    new.append(wall)
                    parts.append(st)
                    out["laps_ms"] = lp
        os.remove(path)
        out["baseline_split_complete_gather_ms"] = spread(prep)
        out["baseline_check16_ms"] = spread(chk)
        out["baseline_ms"] = spread(old)
    out["check_events_ms"] = spread(new)
    for f in ("h2d_ms", "split_ms", "check_ms"):
        out[f] = spread([s[f] for s in parts])
    for f in ("n_client", "n_ops", "n_fail_pairs", "n_ignored_completions", "n_big_keys"):
        out[f] = parts[-1][f]
    out["reps"] = reps
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
