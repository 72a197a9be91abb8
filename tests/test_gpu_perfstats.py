"""lc_perf_stats on the GPU against lc_perf_stats_host: every output array and
every summary counter equal, at the smallest shapes where the kernels can go
wrong.  The shapes are planted in process-sorted order (a slot is a client
event's place in that order): pairs that straddle the wave, the workgroup and
the chunk of the pair pass, neighbours that must not pair at the same places,
the tables round the LDS bound, quantile groups round the wave and the
selection kernel's workgroup, the extreme times and process ids; then
workspace reuse, the resident grid before and after, and one history in bulk."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN
from jepsen.etcd_amd import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "perfstats_kat.json")))["cases"]
COUNTERS = ("valid", "n_events", "n_client", "n_pairs", "n_pending", "n_ignored_completions", "n_mismatched_f",
            "count", "ok", "fail", "info", "t_max", "n_rate_buckets", "n_quant_buckets")
TABLES = ("by_f", "rate", "quant", "quant_n", "comp_pos", "latency_ns")
LIM = abi.perf_stats_limits()
WAVE, BLOCK, CHUNK, MAX_GRID = LIM["wave"], LIM["block"], LIM["chunk"], LIM["max_grid"]
assert (WAVE, BLOCK, CHUNK) == (64, 256, 2048)  # csrc/perfstats.h: kWave, kBlock, kChunk
INV, OK, FAIL, INFO = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def agree(ctx, events, n_f, what="", **kw):
    want, ws = abi.perf_stats_host(events, n_f, **kw)
    got, gs = ctx.perf_stats(events, n_f, **kw)
    for name in TABLES:
        if want[name] is None:
            assert got[name] is None, (what, name)
            continue
        assert want[name].shape == got[name].shape, (what, name, want[name].shape, got[name].shape)
        bad = np.argwhere(want[name] != got[name])
        assert len(bad) == 0, (what, name, bad[:5].tolist(), want[name][tuple(bad[0])], got[name][tuple(bad[0])])
    assert [gs[k] for k in COUNTERS] == [ws[k] for k in COUNTERS], (what, gs, ws)
    return got, gs


def history(procs, n_f=3, seed=1, nemesis=0, ids=None, dt=7):
    """procs: per process the types of its events, in order.  The processes'
    ids ascend (ids, or 2 k + 1), so the slots are the concatenation of procs;
    the history interleaves the processes at random, each in its own order,
    with `nemesis` records that are nobody's strewn in.  A pair shares its f;
    times mostly ascend with the position, with steps back."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(p) for p in procs], dtype=np.int64)
    n_client = int(lens.sum())
    n = n_client + nemesis
    where = rng.permutation(n)
    client_pos, nemesis_pos = where[:n_client], where[n_client:]
    ev = np.zeros(n, dtype=abi.PS_EVENT_DTYPE)
    ev["time"] = np.arange(n) * dt + rng.integers(0, 3 * dt, size=n)
    ev["process"][nemesis_pos] = -1 - rng.integers(0, 3, size=nemesis)
    ev["f"][nemesis_pos] = 9
    ev["type"][nemesis_pos] = rng.integers(0, 4, size=nemesis)
    start = 0
    for k, types in enumerate(procs):
        pos = np.sort(client_pos[start:start + len(types)])
        start += len(types)
        ev["process"][pos] = ids[k] if ids is not None else 2 * k + 1
        ev["type"][pos] = types
        f = rng.integers(0, n_f, size=len(types))
        for j in range(1, len(types)):
            if types[j] != INV and types[j - 1] == INV and rng.random() > 0.05:  # (a few mismatched)
                f[j] = f[j - 1]
        ev["f"][pos] = f
    return ev


def planted(n_client, at, pair):
    """Processes whose slots number n_client, filled with pairs, with slot at -
    1 an invoke and slot `at` a completion: of one process (a pair) or of two
    (a process that ends in an invoke, the next beginning with a completion)."""
    procs = [[INV, OK]] * ((at - 1) // 2)
    if (at - 1) % 2:
        procs = procs + [[FAIL]]
    procs = procs + ([[INV, OK]] if pair else [[INV], [INFO]])
    rest = n_client - at - 1
    procs = procs + [[INV, FAIL]] * (rest // 2) + ([[INV]] if rest % 2 else [])
    assert sum(len(p) for p in procs) == n_client
    return procs


EDGES = sorted({WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1})


def test_nothing_for_the_device(ctx):
    none = np.zeros(0, dtype=abi.PS_EVENT_DTYPE)
    agree(ctx, none, 1, "no events")
    nemesis = np.zeros(300, dtype=abi.PS_EVENT_DTYPE)
    nemesis["process"] = -1
    nemesis["time"] = np.arange(300)
    _, s = agree(ctx, nemesis, 1, "no client events")
    assert s["kernel_ms"] == 0 and s["n_client"] == 0  # (the host code's answer)
    one = history([[OK]])
    _, s = agree(ctx, one, 3, "one event")
    assert s["kernel_ms"] == 0 and s["n_ignored_completions"] == 1


@pytest.mark.parametrize("n_client", EDGES)
def test_pairs_and_neighbours_at_every_edge(ctx, n_client):
    for at in (WAVE, BLOCK, CHUNK):
        if at >= n_client:
            continue
        for pair in (True, False):
            ev = history(planted(n_client, at, pair), nemesis=n_client // 9, seed=at + pair)
            _, s = agree(ctx, ev, 3, (n_client, at, pair), rate_dt_ns=500, quant_dt_ns=900)
            assert s["n_client"] == n_client and s["kernel_ms"] > 0
    # the last slot an invoke: nothing follows it
    procs = [[INV, OK]] * ((n_client - 1) // 2) + ([[FAIL]] if (n_client - 1) % 2 else []) + [[INV]]
    _, s = agree(ctx, history(procs, seed=n_client), 3, (n_client, "ends in an invoke"), rate_dt_ns=500,
                 quant_dt_ns=900)
    assert s["n_pending"] == 1 and s["n_pairs"] == (n_client - 1) // 2
    # the last slot a completion whose invoke is the slot before it
    procs = [[INV, OK]] * ((n_client - 2) // 2) + ([[INFO]] if n_client % 2 else []) + [[INV, OK]]
    _, s = agree(ctx, history(procs, seed=n_client), 3, (n_client, "ends in a pair"), rate_dt_ns=500, quant_dt_ns=900)
    assert s["n_pending"] == 0 and s["n_pairs"] == n_client // 2


def test_one_process_and_every_event_its_own(ctx):
    rng = np.random.default_rng(5)
    types = rng.integers(0, 4, size=CHUNK + BLOCK + 3).tolist()
    _, s = agree(ctx, history([types], nemesis=100), 3, "one process", rate_dt_ns=1000, quant_dt_ns=2000)
    assert s["n_pairs"] > 300 and s["n_pending"] > 100 and s["n_ignored_completions"] > 300
    _, s = agree(ctx, history([[t] for t in types]), 3, "all their own", rate_dt_ns=1000, quant_dt_ns=2000)
    assert s["n_pairs"] == 0 and s["n_pending"] + s["n_ignored_completions"] == len(types)


def test_the_largest_process_id_next_to_process_0(ctx):
    top = 2 ** 31 - 1
    for procs in ([[INV], [OK]], [[INV, OK], [INV, OK]], [[INV, INV], [OK, OK]]):
        agree(ctx, history(procs, ids=[0, top], nemesis=3), 3, procs)
    procs = planted(BLOCK + 1, BLOCK, False)
    agree(ctx, history(procs, ids=list(range(len(procs) - 1)) + [top]), 3, "the last slot is the top id's")


def spread(n, t_max, n_f, seed):
    """n events in pairs on 50 processes, times spread over [0, t_max] with t_max met."""
    rng = np.random.default_rng(seed)
    ev = history([[INV, OK, INV, FAIL, INV, INFO][:6] * (n // 300 + 1)] * 50, n_f=n_f, seed=seed)[:n]
    ev["time"] = rng.integers(0, t_max + 1, size=len(ev))
    ev["time"][len(ev) // 2] = t_max
    return ev


@pytest.mark.parametrize("bound,t_max,rate_dt,quant_dts", [
    (96, 3099, 100, (2000, 1500, 1000)),         # 3 * 31 + 2, + 3, + 4 entries
    (None, 2729, 1, (3000, 2000, 1000)),         # 3 * 2730 + 1, + 2, + 3
])
def test_tables_round_the_lds_bound(ctx, monkeypatch, bound, t_max, rate_dt, quant_dts):
    if bound is not None:
        monkeypatch.setenv("LC_PS_LDS_ENTRIES", str(bound))
    lds = abi.perf_stats_limits()["lds_entries"]
    assert lds == (bound or LIM["default_lds_entries"])
    ev = spread(4000, t_max, 1, seed=t_max)
    for quant_dt, entries in zip(quant_dts, (lds - 1, lds, lds + 1)):
        _, s = agree(ctx, ev, 1, (bound, quant_dt), rate_dt_ns=rate_dt, quant_dt_ns=quant_dt)
        assert 3 * s["n_rate_buckets"] + s["n_quant_buckets"] == entries


def test_global_memory_counts(ctx, monkeypatch):
    monkeypatch.setenv("LC_PS_LDS_ENTRIES", "0")
    assert abi.perf_stats_limits()["lds_entries"] == 0
    agree(ctx, spread(5000, 99999, 7, seed=2), 7, "no LDS at all", rate_dt_ns=1000, quant_dt_ns=3000)
    monkeypatch.delenv("LC_PS_LDS_ENTRIES")
    agree(ctx, spread(5000, 99999, 7, seed=2), 7, "the same in the LDS", rate_dt_ns=1000, quant_dt_ns=3000)
    agree(ctx, spread(3000, 10 ** 6, 40, seed=3), 40, "above the default bound", rate_dt_ns=1000, quant_dt_ns=1000)


def test_one_f_and_max_f(ctx):
    agree(ctx, spread(700, 5000, 1, seed=4), 1, "n_f = 1", rate_dt_ns=100, quant_dt_ns=100)
    ev = spread(700, 5000, 1, seed=4)
    ev["f"] = np.where(np.arange(len(ev)) % 3 == 0, LIM["max_f"] - 1, np.arange(len(ev)) % 5)
    _, s = agree(ctx, ev, LIM["max_f"], "n_f = max_f", rate_dt_ns=5001, quant_dt_ns=2501)
    assert (s["n_rate_buckets"], s["n_quant_buckets"]) == (1, 2)


def pairs_history(pairs, seed=0):
    """pairs: (f, invoke time, latency), each on a process of its own, the
    invokes and the completions in a shuffled order."""
    rng = np.random.default_rng(seed)
    n = len(pairs)
    order = rng.permutation(n)
    ev = np.zeros(2 * n, dtype=abi.PS_EVENT_DTYPE)
    for k, i in enumerate(order):
        f, t, lat = pairs[i]
        ev[k] = (t, 5 * i, f, INV, 0)
        ev[n + k] = (t + lat, 5 * i, f, OK, 0)
    return ev


def test_quantile_groups(ctx):
    rng = np.random.default_rng(9)
    for size in (1, 2, WAVE, WAVE + 1):
        lats = rng.integers(1, 10 ** 6, size=size).tolist()
        pairs = [(1, 100 + i, lats[i]) for i in range(size)] + [(0, 5, 50), (2, 10 ** 6 + 7, 1)]
        got, s = agree(ctx, pairs_history(pairs), 3, ("a group of", size), rate_dt_ns=10 ** 5, quant_dt_ns=10 ** 5)
        assert got["quant_n"][1, 0] == size and got["quant"][1, 0].tolist()[-1] == max(lats)
    got, s = agree(ctx, pairs_history([(0, 10 * b + 3, 1000 + b) for b in range(200)]), 1, "200 groups of one",
                   rate_dt_ns=10, quant_dt_ns=10)
    assert (got["quant_n"][0, :200] == 1).all() and got["quant"][0, 17].tolist() == [1017] * 4
    got, _ = agree(ctx, pairs_history([(0, i, 12345) for i in range(150)]), 1, "all latencies equal",
                   rate_dt_ns=10 ** 6, quant_dt_ns=10 ** 6)
    assert got["quant"][0, 0].tolist() == [12345] * 4
    high = (rng.permutation(150) + 1) << 33
    got, _ = agree(ctx, pairs_history([(0, i, int(high[i])) for i in range(150)]), 1, "only above bit 32",
                   rate_dt_ns=2 ** 42, quant_dt_ns=2 ** 42)
    assert got["quant"][0, 0].tolist() == [76 << 33, 143 << 33, 149 << 33, 150 << 33]
    got, _ = agree(ctx, pairs_history([(0, 1000, -5), (0, 1001, 3), (0, 1002, 9), (0, 1003, -700)]), 1,
                   "negative latencies at the low end", qs=[0.0, 0.25, 0.5, 1.0], rate_dt_ns=10 ** 4,
                   quant_dt_ns=10 ** 4)
    assert got["quant"][0, 0].tolist() == [-700, -5, 3, 9]
    # 250 groups of one, then a group of 20 across the selection kernel's workgroup boundary (slot 256)
    pairs = [(0, 10 * b, 7 + b) for b in range(250)] + [(0, 2500 + (i % 10), 100 - i) for i in range(20)]
    got, _ = agree(ctx, pairs_history(pairs), 1, "a group across the workgroup", rate_dt_ns=10, quant_dt_ns=10)
    assert got["quant_n"][0, 250] == 20 and got["quant"][0, 250].tolist() == [91, 100, 100, 100]


def test_no_quantile_and_eight(ctx):
    ev = spread(3000, 10 ** 5, 3, seed=6)
    got, _ = agree(ctx, ev, 3, "n_q = 0", qs=[], rate_dt_ns=1000, quant_dt_ns=5000)
    assert got["quant"].shape == (3, 21, 0) and got["quant_n"].sum() > 1000
    agree(ctx, ev, 3, "n_q = 8", qs=[0.0, 0.1, 0.5, 0.75, 0.95, 0.99, 0.999, 1.0], rate_dt_ns=1000, quant_dt_ns=5000)


def test_times_at_2_to_the_62(ctx):
    ev = history(planted(BLOCK + 5, BLOCK, True), seed=8)
    ev["time"] += 2 ** 62
    _, s = agree(ctx, ev, 3, "2^62", rate_dt_ns=2 ** 58, quant_dt_ns=2 ** 60)
    assert s["t_max"] > 2 ** 62 and (s["n_rate_buckets"], s["n_quant_buckets"]) == (17, 5)
    ev["time"][::2] -= 2 ** 62  # latencies of about +- 2^62
    agree(ctx, ev, 3, "0 and 2^62", rate_dt_ns=2 ** 58, quant_dt_ns=2 ** 60)


def test_bucket_boundaries(ctx):
    dt = 1000
    pairs = [(0, k * dt - 1, 1) for k in range(1, 40)] + [(0, k * dt, dt - 1) for k in range(1, 40)] + \
            [(1, k * dt, dt) for k in range(40)]
    got, s = agree(ctx, pairs_history(pairs), 2, "k dt and k dt - 1", rate_dt_ns=dt, quant_dt_ns=dt)
    assert got["quant_n"][0, :40].tolist() == [1] + [2] * 38 + [1] and s["n_quant_buckets"] == 41


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(ctx, kat):
    ev = np.zeros(len(kat["events"]), dtype=abi.PS_EVENT_DTYPE)
    for i, (t, p, f, ty) in enumerate(kat["events"]):
        ev[i] = (t, p, f, ty, 0)
    got, s = agree(ctx, ev, kat["n_f"], kat["name"], qs=kat["qs"], rate_dt_ns=kat["rate_dt"],
                   quant_dt_ns=kat["quant_dt"])
    assert all(got[name].tolist() == kat[name] for name in TABLES) and {k: s[k] for k in COUNTERS} == kat["summary"]


def test_without_the_point_arrays(ctx):
    ev = history(planted(CHUNK + 1, CHUNK, True), nemesis=50)
    with_points, _ = agree(ctx, ev, 3, "points", rate_dt_ns=1000, quant_dt_ns=3000)
    without, _ = agree(ctx, ev, 3, "no points", rate_dt_ns=1000, quant_dt_ns=3000, points=False)
    assert without["comp_pos"] is None and without["latency_ns"] is None
    assert all((with_points[k] == without[k]).all() for k in ("by_f", "rate", "quant", "quant_n"))


def test_refusals_leave_the_context_usable(ctx):
    good = history(planted(BLOCK + 1, BLOCK, True))
    for what, change, code in (("time", lambda e: e["time"].__setitem__(200, -1), -22),
                               ("type", lambda e: e["type"].__setitem__(BLOCK, 4), -22),
                               ("f", lambda e: e["f"].__setitem__(0, 3), -22)):
        ev = good.copy()
        change(ev)
        with pytest.raises(abi.LcError) as e:
            ctx.perf_stats(ev, 3)
        assert e.value.code == code and "lc_perf_stats" in str(e.value), what
        agree(ctx, good, 3, "after " + what)
    with pytest.raises(abi.LcError) as e:
        ctx.perf_stats(good, 3, rate_dt_ns=1, quant_dt_ns=1, rate_cap=5, quant_cap=10 ** 4)
    want = int(good["time"][good["process"] >= 0].max()) + 1
    assert e.value.code == -28 and e.value.needed == (want, want)
    agree(ctx, good, 3, "with room", rate_dt_ns=1, quant_dt_ns=1, rate_cap=want, quant_cap=want + 3)
    with pytest.raises(abi.LcError) as e:
        ctx.perf_stats(good, LIM["max_f"], rate_dt_ns=1, quant_dt_ns=1)
    assert e.value.code == -7


def test_workspace_reuse():
    """Many fs and few events, then few fs and many events, then the first
    again, on a fresh context: the tables shrink and the per-event arrays grow
    inside an arena the first call sized, and back."""
    many_f = spread(900, 40000, 5000, seed=11)
    many_events = history([[INV, OK, INV, FAIL] * 500] * 100, n_f=2, seed=12, nemesis=3000)
    assert len(many_events) == 203000
    with abi.Context(device_mask=1) as c:
        for what, ev, n_f in (("many fs", many_f, 5000), ("many events", many_events, 2),
                              ("many fs again", many_f, 5000), ("many events again", many_events, 2)):
            agree(c, ev, n_f, what, rate_dt_ns=10000, quant_dt_ns=20000)


def test_the_register_path_before_and_after(monkeypatch):
    """lc_check_device on the same context before and after lc_perf_stats,
    with the resident grid kept alive in between: the side checker has to stop
    it, and the register path's results do not change."""
    import torch
    monkeypatch.setenv("LC_RESIDENT_IDLE_US", "200000")
    z = np.load(os.path.join(GOLDEN, "c1.npz"))
    n = min(len(z["key_off"]) - 1, 1200)
    dev = torch.device("cuda", 0)
    d_ops = torch.from_numpy(np.ascontiguousarray(z["ops"][:z["key_off"][n]])).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(z["key_off"][:n + 1])).to(dev)

    def register(c):
        d_out = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
        c.check_device(d_ops.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(),
                       stream=torch.cuda.current_stream(dev).cuda_stream)
        return np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=abi.RESULT_DTYPE)[:n].copy()

    ev = history(planted(CHUNK + 1, CHUNK, True), nemesis=50)
    with abi.Context(device_mask=1) as c:
        before = register(c)
        assert (before["verdict"] == z["verdict"][:n]).all()
        register(c)
        agree(c, ev, 3, "between register calls", rate_dt_ns=1000, quant_dt_ns=3000)
        after = register(c)
        agree(c, ev, 3, "again", rate_dt_ns=1000, quant_dt_ns=3000)
        assert (after == before).all()


def test_bulk(ctx):
    """About a million events on 100 processes with 8 fs: more chunks than the
    pair pass has workgroups only by its grid stride's count, more slots than
    the other kernels' grids hold at once."""
    rng = np.random.default_rng(2024)
    n, n_proc, n_f = 1_000_000, 100, 8
    assert n > MAX_GRID * BLOCK
    ev = np.zeros(n, dtype=abi.PS_EVENT_DTYPE)
    ev["process"] = rng.integers(0, n_proc, size=n)
    ev["process"][rng.random(n) < 0.01] = -1
    ev["time"] = np.cumsum(rng.integers(0, 200_000, size=n))  # about 100 s in all
    # each process alternates invoke and completion, with a few slips
    order = np.argsort(ev["process"], kind="stable")
    ty = np.tile(np.array([INV, OK], dtype=np.uint8), n // 2)
    comp = rng.random(n)
    ty = np.where((ty != INV) & (comp < 0.05), FAIL, ty)
    ty = np.where((ty != INV) & (comp > 0.97), INFO, ty)
    ty = np.where(rng.random(n) < 0.002, INV, ty)
    ev["type"][order] = ty
    f = rng.integers(0, n_f, size=n // 2).repeat(2)
    ev["f"][order] = np.where(rng.random(n) < 0.002, rng.integers(0, n_f, size=n), f)  # (some pairs mismatched)
    got, s = agree(ctx, ev, n_f, "bulk")
    assert s["n_pairs"] > 480_000 and s["n_pending"] > 500 and s["n_mismatched_f"] > 100
    assert s["n_rate_buckets"] > 5 and s["valid"] == 1
