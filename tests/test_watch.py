"""lc_watch_check_host and jepsen/etcd_amd/watch.py against the hand-derived
cases of tests/golden/watch_kat.json and against tests/watch_ref.py, an
independent restatement (LCS-table distances, tuple-equality classes, its own
Myers and patch).  No GPU."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import watch_ref as R
from jepsen.etcd_amd import abi, watch as W

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "watch_kat.json")))["cases"]


def arrays(logs, revisions=None, ids=None):
    threads = np.zeros(len(logs), dtype=abi.WT_THREAD_DTYPE)
    off = 0
    for i, log in enumerate(logs):
        threads[i] = (off, len(log), revisions[i] if revisions else 1, ids[i] if ids else i)
        off += len(log)
    return threads, np.array([x for log in logs for x in log], dtype=np.int64).reshape(-1)


def logs_of(threads, values):
    return [[int(v) for v in values[int(t["off"]):int(t["off"] + t["len"])]] for t in threads]


def script_of(out, d):
    return [(int(e["op"]), int(e["at"]), int(e["value"]))
            for e in out["edits"][int(d["script_off"]):int(d["script_off"] + d["script_len"])]]


def assert_matches_ref(out, s, logs, revisions, n_nonmonotonic=0, max_d=4096):
    ref = R.check(logs, revisions, n_nonmonotonic, max_d)
    assert out["cls"].tolist() == ref["cls"]
    assert s["canonical"] == (-1 if ref["canonical"] is None else ref["canonical"])
    assert (s["canonical_size"], s["n_classes"], s["n_threads"]) == (ref["canonical_size"], ref["n_classes"], len(logs))
    assert out["distance"].tolist() == ref["distance"]
    assert {1: True, 0: False, -1: "unknown"}[s["valid"]] == ref["valid"]
    assert s["revisions_equal"] == int(len(set(revisions)) <= 1)
    assert s["n_deltas"] == len(ref["deltas"]) == len(out["deltas"])
    off = 0
    for d, (t, dist, p, sfx, script) in zip(out["deltas"], ref["deltas"]):
        assert (int(d["thread"]), int(d["edit_distance"]), int(d["prefix"]), int(d["suffix"])) == (t, dist, p, sfx)
        A, B = logs[ref["canonical"]], logs[t]
        assert p + sfx <= min(len(A), len(B))
        if script is None:
            assert (int(d["flags"]), int(d["script_len"])) == (abi.LC_WT_NO_SCRIPT, 0)
            continue
        got = script_of(out, d)
        assert (int(d["flags"]), int(d["script_off"]), int(d["script_len"])) == (0, off, dist) and len(got) == dist
        off += dist
        assert all(x[1] <= y[1] for x, y in zip(got, got[1:]))  # `at` never decreases
        assert R.patch(A, got) == B
        assert got == script  # rule 5, entry for entry
    assert s["n_edits"] == off == len(out["edits"])
    assert s["n_no_script"] == sum(1 for d in ref["deltas"] if d[4] is None)


def _int_keys(m):
    return {int(k): v for k, v in m.items()}


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_known_answers_through_the_checker(kat):
    got = W.WatchChecker(use_gpu=False).check({"concurrency": kat["concurrency"]}, kat["history"], {})
    want = dict(kat["expect"])
    for k in ("revisions", "logs"):
        if k in want:
            want[k] = _int_keys(want[k])
    assert got == want, kat["why"]


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_known_answers_host_against_the_reference(kat):
    enc = W.encode(kat["history"], kat["concurrency"])
    out, s = abi.watch_check_host(enc.threads, enc.values, len(enc.nonmonotonic))
    assert_matches_ref(out, s, logs_of(enc.threads, enc.values), enc.threads["revision"].tolist(), len(enc.nonmonotonic))


def test_encode_refuses_a_watch_without_a_log():
    with pytest.raises(W.Unsupported):
        W.encode([{"type": "ok", "f": "watch", "process": 0, "value": {"revision": 1}}], 2)


def random_logs(rng):
    """2-9 threads, logs of 0-40 values over 2-4 symbols: some equal, some a few edits apart, some unrelated."""
    syms = rng.randint(2, 4)
    base = [rng.randrange(syms) for _ in range(rng.randint(0, 40))]
    logs = []
    for _ in range(rng.randint(2, 9)):
        c = rng.random()
        if c < 0.35:
            log = list(base)
        elif c < 0.8:
            log = list(base)
            for _ in range(rng.randint(1, 4)):
                at = rng.randrange(len(log) + 1)
                if rng.random() < 0.5 and at < len(log):
                    del log[at]
                elif len(log) < 40:
                    log.insert(at, rng.randrange(syms))
        else:
            log = [rng.randrange(syms) for _ in range(rng.randint(0, 40))]
        logs.append(log)
    return logs


def test_two_thousand_random_inputs_against_the_reference():
    rng = random.Random(0x57A7C4)
    seen = {True: 0, False: 0, "unknown": 0}
    for i in range(2000):
        logs = random_logs(rng)
        revisions = [5] * len(logs)
        if rng.random() < 0.1:
            revisions[rng.randrange(len(logs))] = 6
        nn = 1 if rng.random() < 0.05 else 0
        threads, values = arrays(logs, revisions)
        out, s = abi.watch_check_host(threads, values, nn)
        assert_matches_ref(out, s, logs, revisions, nn)
        seen[{1: True, 0: False, -1: "unknown"}[s["valid"]]] += 1
    assert all(n > 20 for n in seen.values()), seen


def test_the_reference_s_myers_agrees_with_its_lcs_table():
    rng = random.Random(7)
    for _ in range(3000):
        a = [rng.randrange(3) for _ in range(rng.randint(0, 12))]
        b = [rng.randrange(3) for _ in range(rng.randint(0, 12))]
        sc = R.myers(a, b)
        assert len(sc) == R.distance(a, b) and R.patch(a, sc) == b
        assert all(x[1] <= y[1] for x, y in zip(sc, sc[1:]))


@pytest.mark.parametrize("A, B", [([1, 1, 1], [1, 1, 1, 1]), ([1, 1, 1, 1], [1, 1, 1]), ([1] * 70, [1] * 5),
                                  ([1, 2, 1, 2, 1], [1, 2, 1]), ([2, 1, 1], [1, 1])])
def test_prefix_and_suffix_never_overlap(A, B):
    logs = [A, A, B]
    out, s = abi.watch_check_host(*arrays(logs))
    d = out["deltas"][0]
    assert int(d["prefix"]) + int(d["suffix"]) <= min(len(A), len(B))
    assert_matches_ref(out, s, logs, [1, 1, 1])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_max_d_at_the_distance_and_beside_it(monkeypatch, delta):
    A = list(range(100, 130))
    B = [x for x in A if x % 5] + [7, 8]  # 6 deletions and 2 insertions: D = 8
    logs = [A, A, B]
    assert R.distance(A, B) == 8
    monkeypatch.setenv("LC_WT_MAX_D", str(8 + delta))
    assert abi.watch_limits()["max_d"] == 8 + delta
    out, s = abi.watch_check_host(*arrays(logs))
    d = out["deltas"][0]
    assert int(d["edit_distance"]) == 8  # exact either way
    assert (int(d["flags"]) == abi.LC_WT_NO_SCRIPT) == (delta < 0)
    assert s["n_no_script"] == int(delta < 0) and s["n_edits"] == (0 if delta < 0 else 8)
    assert_matches_ref(out, s, logs, [1, 1, 1], max_d=8 + delta)


def test_limits_and_their_overrides(monkeypatch):
    lim = abi.watch_limits()
    assert (lim["max_d"], lim["trace_bytes"], lim["max_len"], lim["hash_mask"]) == (4096, 2 ** 30, 2 ** 31 - 1, 2 ** 64 - 1)
    monkeypatch.setenv("LC_WT_MAX_D", "100000")
    monkeypatch.setenv("LC_WT_TRACE_BYTES", "4096")
    monkeypatch.setenv("LC_WT_HASH_MASK", "0x1")
    lim = abi.watch_limits()
    assert (lim["max_d"], lim["trace_bytes"], lim["hash_mask"]) == (abi.LC_WT_MAX_D_LIMIT, 4096, 1)


@pytest.mark.parametrize("mask", ["0", "1"])
def test_forced_hash_collisions_leave_the_classes_exact(monkeypatch, mask):
    logs = [[1, 2, 3], [1, 2, 4], [1, 2, 3], [5, 2, 3], [1, 2, 4]]  # 5 threads in 3 classes, one length
    monkeypatch.setenv("LC_WT_HASH_MASK", mask)
    out, s = abi.watch_check_host(*arrays(logs))
    assert_matches_ref(out, s, logs, [1] * 5)
    assert s["n_classes"] == 3 and s["n_collisions"] > 0


def test_enospc_names_the_room_and_the_retry_succeeds():
    logs = [[1, 2, 3, 4], [1, 2, 3, 4], [1, 3, 2, 4], [1, 2, 3]]
    threads, values = arrays(logs)
    with pytest.raises(abi.LcError) as e:
        abi.watch_check_host(threads, values, edit_cap=2)
    assert e.value.code == -28 and e.value.n_edits == 3
    out, s = abi.watch_check_host(threads, values, edit_cap=3)
    assert s["n_edits"] == 3
    assert_matches_ref(out, s, logs, [1] * 4)


def _raw(threads, values, n_values=None, flags=0):
    call = abi._WatchCall(threads, values, 0, flags)
    args = list(call.args())
    if n_values is not None:
        args[3] = n_values
    before = {k: v.copy() for k, v in call.arrays.items()}
    rc = abi.lib().lc_watch_check_host(*args)
    assert all((call.arrays[k] == before[k]).all() for k in before)  # nothing written
    return rc


def test_refusals():
    threads, values = arrays([[1, 2], [1, 2]])
    assert _raw(threads, values) == 0
    assert _raw(threads, values, flags=1) == -22  # an unknown flag
    t = threads.copy()
    t[1]["thread"] = t[0]["thread"]
    assert _raw(t, values) == -22  # a thread id repeated
    for field, v in (("off", -1), ("len", -1), ("off", 3), ("len", 3)):
        t = threads.copy()
        t[1][field] = v
        assert _raw(t, values) == -22, (field, v)  # negative, or past n_values
    t = threads.copy()
    t[1]["off"], t[1]["len"] = 0, 2 ** 31 - 1
    assert _raw(t, values, n_values=2 ** 31) == -22  # a log of 2^31 - 1 entries
    assert abi.lib().lc_watch_limits(ctypes.POINTER(abi.LcWtLimits)()) == -22


def test_synth_arrays_make_what_they_say():
    threads, values = W.synth_arrays(5, 200, {1: 3, 4: 1}, seed=3)
    out, s = abi.watch_check_host(threads, values)
    assert s["canonical"] == 0 and s["canonical_size"] == 3 and s["n_deltas"] == 2
    assert 1 <= out["distance"][1] <= 6 and 1 <= out["distance"][4] <= 2


def test_the_checker_omits_a_diff_above_the_cap(monkeypatch):
    kat = next(k for k in KATS if k["name"] == "two-swapped")
    monkeypatch.setenv("LC_WT_MAX_D", "1")
    got = W.WatchChecker(use_gpu=False).check({"concurrency": 3}, kat["history"], {})
    assert got["deltas"] == [{"thread": 2, "edit-distance": 2, "diff": None, "diff-omitted": True}]
    assert got["canonical"] == [1, 2, 3, 4] and got["valid?"] is False
