"""Histories with one stale read planted, as lc_append_check's and
lc_wr_check's arrays: what tools/screen_probe.py's stale_append / stale_wr do
to its 10^6-txn histories, restated for small ones.  The base history is
append.synth_arrays / wr.synth_arrays (valid, every txn completes) with about
`conc` txns overlapping (1: sequential); one late read then answers as a read
did `back` txns before it, which closes one G-single-realtime cycle through
about `back` txns.  "Before it" counts the txns that completed before the
reader's invoke: a txn that overlaps the reader is not in its past, and a read
that repeats it is not stale (in a sequential history the two counts are one).
The reader is the last one for which the host checker finds the cycle; the
plant is a function of its arguments alone."""
import numpy as np

from jepsen.etcd_amd import abi, append as AP, wr as WR

BACKS = (2, 63, 64, 65, 300)
CONCS = (1, 8)
N_TXNS = 700


def _late_reads(txns, mops, is_read):
    """The reads by OK txns that are alone in their txn, the last first: (txn, mop, the OK txns completed before its invoke)."""
    ok = np.nonzero(txns["type"] == abi.LC_AP_OK)[0]
    for t in range(len(txns) - 1, -1, -1):
        m = int(txns["mop_off"][t])
        if txns["type"][t] == abi.LC_AP_OK and txns["mop_len"][t] == 1 and is_read(m):
            yield t, m, ok[txns["comp_pos"][ok] < txns["inv_pos"][t]]


def _one_cycle(s):
    return s["n_scc"] == 1 and s["n_class"][6] == 1


def stale_append(txns, mops, values, back):
    """A late read answers as a non-empty read did in one of the `back` txns
    last completed before it (the earliest such): a prefix of a key that has
    grown since."""
    for t, m, done in _late_reads(txns, mops, lambda m: mops["f"][m] == abi.LC_AP_READ and mops["len"][m] >= 0):
        if len(done) < back:
            break
        for u in done[-back:]:
            lo, hi = int(txns["mop_off"][u]), int(txns["mop_off"][u]) + int(txns["mop_len"][u])
            early = [i for i in range(lo, hi) if mops["f"][i] == abi.LC_AP_READ and mops["len"][i] >= 1]
            if not early:
                continue
            bad = mops.copy()
            bad[m] = mops[early[0]]
            if _one_cycle(abi.append_check_host(txns, bad, values)[1]):
                return txns, bad, values
            break  # (this reader's earliest candidate closes nothing: an earlier reader)
    raise RuntimeError("no read to make stale")


def stale_wr(txns, mops, back):
    """A late read answers with a value that one of the `back` txns last
    completed before it (the earliest such) read and overwrote."""
    for t, m, done in _late_reads(txns, mops, lambda m: mops["f"][m] == abi.LC_WR_READ and mops["known"][m] == 1):
        if len(done) < back:
            break
        for u in done[-back:]:
            lo, hi = int(txns["mop_off"][u]), int(txns["mop_off"][u]) + int(txns["mop_len"][u])
            early = [i for i in range(lo, hi)
                     if mops["f"][i] == abi.LC_WR_READ and mops["known"][i] and mops["value"][i] != abi.LC_WR_NIL and
                     not (mops["key"][lo:i] == mops["key"][i]).any() and
                     ((mops["key"][i + 1:hi] == mops["key"][i]) & (mops["f"][i + 1:hi] == abi.LC_WR_WRITE)).any()]
            if not early:
                continue
            bad = mops.copy()
            bad["key"][m], bad["value"][m] = mops["key"][early[0]], mops["value"][early[0]]
            if _one_cycle(abi.wr_check_host(txns, bad, True)[1]):
                return txns, bad
            break
    raise RuntimeError("no overwritten read to repeat")


def append_plant(back, conc, n_txns=N_TXNS, seed=1):
    # (long-lived keys, so that the key read `back` txns ago is still appended to)
    return stale_append(*AP.synth_arrays(n_txns, seed=seed, live_keys=2, per_key=n_txns, concurrency=conc, p_info=0.0),
                        back)


def wr_plant(back, conc, n_txns=N_TXNS, seed=1):
    return stale_wr(*WR.synth_arrays(n_txns, seed=seed, live_keys=2, per_key=n_txns, concurrency=conc, p_info=0.0), back)
