"""lc_watch_check on the GPU against lc_watch_check_host: every output array
and every count equal, at the smallest shapes where the kernels can go wrong:
thread counts and log lengths round the wave, the compare's tile and the
workgroup's stride; one differing element on each side of every such boundary,
from the front and from the end; prefixes and suffixes that would overlap;
empty middles; snakes round the lone-lane step count and the cooperative
strides; distances round the wave and the cap; two batches of traces; forced
hash collisions; the extreme values; workspace reuse; the known-answer cases;
and in bulk."""
import json
import os
import random

import numpy as np
import pytest

import watch_ref as R
from jepsen.etcd_amd import abi, watch as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "watch_kat.json")))["cases"]
COUNTS = ("valid", "canonical", "canonical_size", "n_threads", "n_classes", "n_deltas", "n_edits", "n_no_script",
          "n_collisions", "revisions_equal")
LONE, TILE, STRIDE, HASH_GROUP = 8, 256, 1024, 2048  # watch.h: kLone, kTile, kStride; watch.hip: kHashUnroll x kBlock


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def arrays(logs, revisions=None):
    threads = np.zeros(len(logs), dtype=abi.WT_THREAD_DTYPE)
    off = 0
    for i, log in enumerate(logs):
        threads[i] = (off, len(log), revisions[i] if revisions else 1, i)
        off += len(log)
    values = np.concatenate([np.asarray(log, dtype=np.int64).reshape(-1) for log in logs]) if logs else []
    return threads, np.asarray(values, dtype=np.int64)


def agree_arrays(ctx, threads, values, nn=0, what=""):
    want, ws = abi.watch_check_host(threads, values, nn)
    got, gs = ctx.watch_check(threads, values, nn)
    for f in want:
        assert want[f].shape == got[f].shape, (what, f, want[f].shape, got[f].shape)
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), want[f][bad[:3]].tolist(), got[f][bad[:3]].tolist())
    assert [gs[k] for k in COUNTS] == [ws[k] for k in COUNTS], (what, gs, ws)
    assert gs["n_by_host"] == gs["n_no_script"] and ws["n_by_host"] == 0
    return got, gs


def agree(ctx, logs, revisions=None, nn=0, what=""):
    return agree_arrays(ctx, *arrays(logs, revisions), nn=nn, what=what)


def base_log(n, seed=1):
    return np.random.default_rng(seed).integers(1, 2 ** 40, size=n, dtype=np.int64)


def changed(log, *idx):
    out = np.array(log, dtype=np.int64)
    for i in idx:
        out[i] = -out[i] - 1
    return out


@pytest.mark.parametrize("n_threads", [2, 3, 63, 64, 65, 257])
def test_thread_counts(ctx, n_threads):
    base = base_log(70)
    logs = [changed(base, (7 * t) % 70) if t % 3 == 2 else np.delete(base, t % 70) if t % 5 == 4 else base
            for t in range(n_threads)]
    got, s = agree(ctx, logs, what=n_threads)
    assert s["n_deltas"] == sum(1 for t in range(n_threads) if t % 3 == 2 or t % 5 == 4)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 1, HASH_GROUP - 1,
                               HASH_GROUP, HASH_GROUP + 1, HASH_GROUP + 256])
def test_log_lengths(ctx, n):
    base = base_log(n)
    logs = [base, base, base]
    if n:
        logs += [changed(base, n - 1), changed(base, 0), base[:-1], base[1:]]
    logs += [np.append(base, 5), np.append(5, base)]
    got, s = agree(ctx, logs, what=n)
    assert s["canonical_size"] == 3 and s["n_deltas"] == len(logs) - 3


def test_one_differing_element_on_each_side_of_every_boundary(ctx):
    n = 2 * STRIDE + 77
    base = base_log(n)
    edges = sorted({0, 1, 62, 63, 64, 65, TILE - 1, TILE, TILE + 1, STRIDE - 1, STRIDE, STRIDE + 1, 2 * STRIDE - 1,
                    2 * STRIDE, n - 1})
    logs = [base] * 5  # the equal twins (more of them than of any changed log below)
    for i in edges:
        logs.append(changed(base, i))          # the prefix ends there, the suffix search starts behind it
        logs.append(changed(base, n - 1 - i))  # the same counted from the end
        logs.append(changed(base, i, n - 1 - i) if i < n - 1 - i else changed(base, i))
    got, s = agree(ctx, logs)
    assert s["n_classes"] == len({tuple(log.tolist()) for log in logs})
    for d in got["deltas"]:
        B = logs[int(d["thread"])]
        differ = np.nonzero(B != base)[0]
        assert int(d["prefix"]) == differ[0] and int(d["suffix"]) == n - 1 - differ[-1]


def test_prefix_and_suffix_that_would_overlap(ctx):
    for run in (100, 300):
        logs = [[1] * run, [1] * run, [1] * (run + 1), [1] * (run - 1), [1] * (run + 65), [1] * (run - 65),
                [1] * (run + STRIDE), []]
        got, s = agree(ctx, logs, what=run)
        for d in got["deltas"]:
            assert int(d["prefix"]) + int(d["suffix"]) == min(run, len(logs[int(d["thread"])]))
            assert int(d["edit_distance"]) == abs(run - len(logs[int(d["thread"])]))


def test_all_insert_and_all_delete_middles(ctx):
    base = base_log(500)
    block = base_log(70, seed=2)
    logs = [base, base, np.concatenate([base[:200], block, base[200:]]), np.delete(base, np.arange(200, 270)),
            np.concatenate([block[:3], base]), base[:-64]]
    got, s = agree(ctx, logs)
    assert got["distance"].tolist() == [0, 0, 70, 70, 3, 64]


def snake_rounds(a, b):
    """The forward pass in Python, counting per round the snakes longer than the lone-lane steps."""
    n, m, v, out = len(a), len(b), {1: 0}, []
    for d in range(n + m + 1):
        long_ones = 0
        for k in range(-d, d + 1, 2):
            x = v[k + 1] if k == -d or (k != d and v[k - 1] < v[k + 1]) else v[k - 1] + 1
            x0 = x
            while x < n and x - k < m and a[x] == b[x - k]:
                x += 1
            long_ones += x - x0 > LONE
            v[k] = x
        out.append(long_ones)
        if abs(n - m) <= d and (d - (n - m)) % 2 == 0 and v[n - m] >= n:
            return out


@pytest.mark.parametrize("snake", [LONE - 1, LONE, LONE + 1, TILE - 1, TILE, TILE + 1, STRIDE - 1, STRIDE, STRIDE + 1,
                                   LONE + TILE, LONE + STRIDE - 1, LONE + STRIDE, LONE + STRIDE + 1])
def test_snake_lengths(ctx, snake):
    # after a deletion at 10 the path follows `snake` equal elements, up to a replaced one
    base = base_log(snake + 60)
    B = np.delete(changed(base, 11 + snake), 10)
    got, s = agree(ctx, [base, base, B], what=snake)
    assert got["distance"].tolist() == [0, 0, 3]


def test_two_long_snakes_in_one_round(ctx):
    rng = random.Random(5)
    runs = []
    while sum(runs) < 6000:
        runs.append(rng.randint(300, 700))
    base = np.repeat(np.arange(len(runs)) % 2, runs).astype(np.int64)
    logs = [base, base]
    for t in range(3):
        log = list(base)
        for _ in range(4):
            at = rng.randrange(len(log))
            if rng.random() < 0.5:
                del log[at]
            else:
                log.insert(at, rng.randrange(2))
        logs.append(np.array(log, dtype=np.int64))
    # and one built for it: round 1's two diagonals both run on for 600 elements and more
    period = np.array([1, 2] * 300 + [9, 9, 9], dtype=np.int64)
    shifted = np.array([2, 1] * 300 + [9, 9, 9], dtype=np.int64)
    p, sfx = R.trim(period.tolist(), shifted.tolist())
    assert max(snake_rounds(period[p:len(period) - sfx].tolist(), shifted[p:len(shifted) - sfx].tolist())) >= 2
    got, s = agree(ctx, [period, period, shifted])
    assert got["distance"].tolist() == [0, 0, 2]
    agree(ctx, logs)


def at_distance(base, D, seed):
    """base with ceil(D / 2) deletions and floor(D / 2) insertions of new values: distance D exactly."""
    rng = random.Random(seed)
    gone = sorted(rng.sample(range(len(base)), (D + 1) // 2))
    log = [int(x) for i, x in enumerate(base) if i not in set(gone)]
    for j in range(D // 2):
        log.insert(rng.randrange(len(log) + 1), -1 - j)
    return np.array(log, dtype=np.int64)


def test_distances_round_the_wave(ctx):
    base = base_log(600)
    ds = [1, 2, 63, 64, 65, 130]
    got, s = agree(ctx, [base, base] + [at_distance(base, D, D) for D in ds])
    assert got["distance"].tolist() == [0, 0] + ds and s["n_no_script"] == 0 and s["n_edits"] == sum(ds)
    for d in got["deltas"]:
        sc = got["edits"][int(d["script_off"]):int(d["script_off"] + d["script_len"])]
        script = [(int(e["op"]), int(e["at"]), int(e["value"])) for e in sc]
        assert R.patch(base.tolist(), script) == at_distance(base, int(d["edit_distance"]),
                                                             int(d["edit_distance"])).tolist()


def test_distances_round_the_cap(ctx, monkeypatch):
    monkeypatch.setenv("LC_WT_MAX_D", "64")
    base = base_log(600)
    got, s = agree(ctx, [base, base] + [at_distance(base, D, D) for D in (63, 64, 65)])
    assert got["distance"].tolist() == [0, 0, 63, 64, 65]
    assert (s["n_no_script"], s["n_by_host"], s["n_edits"]) == (1, 1, 127)
    assert got["deltas"]["flags"].tolist() == [abi.LC_WT_NO_SCRIPT, 0, 0]


def test_a_trace_budget_that_forces_two_batches(ctx, monkeypatch):
    base = base_log(300)
    logs = [base, base] + [at_distance(base, D, D) for D in (9, 30, 4, 17, 1)]
    whole, _ = agree(ctx, logs)
    # a thread's trace is sized by min(max_d, len a + len b), here up to about 600 rounds and 0.73 MB:
    # two or three threads to a batch
    monkeypatch.setenv("LC_WT_TRACE_BYTES", "1500000")
    parts, _ = agree(ctx, logs)
    monkeypatch.setenv("LC_WT_TRACE_BYTES", "1")  # every thread alone, each larger than the budget
    single, _ = agree(ctx, logs)
    for f in whole:
        assert (whole[f] == parts[f]).all() and (whole[f] == single[f]).all(), f


@pytest.mark.parametrize("mask", ["0", "1"])
def test_forced_hash_collisions(ctx, monkeypatch, mask):
    a, b, c = base_log(300, 1), base_log(300, 2), changed(base_log(300, 1), 299)
    monkeypatch.setenv("LC_WT_HASH_MASK", mask)
    got, s = agree(ctx, [a, b, a, c, b], what=mask)  # 5 threads in 3 classes, one length
    assert got["cls"].tolist() == [0, 1, 0, 3, 1] and s["n_classes"] == 3 and s["n_collisions"] > 0


def test_extreme_values(ctx):
    lo, hi = -2 ** 63, 2 ** 63 - 1
    base = np.array([lo, hi, 0, -1, lo, lo, hi, 1] * 40, dtype=np.int64)
    swapped = base.copy()
    swapped[5], swapped[6] = hi, lo
    logs = [base, base, swapped, np.delete(base, 4), np.insert(base, 100, hi), np.insert(base, 7, lo)]
    got, s = agree(ctx, logs)
    assert s["n_deltas"] == 4


def test_arena_reuse_shrinking_then_growing(ctx):
    for n, t in ((5000, 9), (40, 3), (9000, 12)):
        threads, values = W.synth_arrays(t, n, {1: 3, 2: 60 if n > 100 else 2}, seed=n)
        agree_arrays(ctx, threads, values, what=n)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(ctx, kat):
    enc = W.encode(kat["history"], kat["concurrency"])
    agree_arrays(ctx, enc.threads, enc.values, nn=len(enc.nonmonotonic), what=kat["name"])
    got = W.WatchChecker(ctx=ctx).check({"concurrency": kat["concurrency"]}, kat["history"], {})
    want = dict(kat["expect"])
    for k in ("revisions", "logs"):
        if k in want:
            want[k] = {int(t): v for t, v in want[k].items()}
    assert got == want, kat["why"]


def test_bulk(ctx):
    rng = random.Random(11)
    edits = {t: rng.randint(0, 5) for t in range(64) if t % 3 == 1}
    threads, values = W.synth_arrays(64, 20000, edits, seed=4)
    got, s = agree_arrays(ctx, threads, values)
    assert s["canonical"] == 0 and s["n_deltas"] == sum(1 for k in edits.values() if k)
    A = values[:20000].tolist()
    for d in got["deltas"]:
        t = threads[int(d["thread"])]
        sc = got["edits"][int(d["script_off"]):int(d["script_off"] + d["script_len"])]
        script = [(int(e["op"]), int(e["at"]), int(e["value"])) for e in sc]
        assert len(script) == int(d["edit_distance"])
        assert R.patch(A, script) == values[int(t["off"]):int(t["off"] + t["len"])].tolist()
