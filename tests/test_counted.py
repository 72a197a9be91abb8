"""The counted-class search tier (LC_FLAG_COUNTED_CLASSES): crashed writes/CAS
are counted per class instead of holding a window slot each, so lc_check
decides version-less keys with more than 64 outstanding crashed mutations.

CPU tests pin the public symbols and the layout rule (lc_counted_plan against
a Python restatement); GPU tests compare every result field with the oracle's
JITC mode, whose window is unbounded."""
import functools
import random

import numpy as np
import pytest

import oracle
from helpers import FREE, INF, C, N, R, W, _intervals, pack_keys, random_casreg, random_mutex
from jepsen.etcd_amd import abi

FIELDS = ("verdict", "reason", "fail_op", "fail_prefix_end", "configs_explored", "max_frontier")
OVERFLOW = abi.LC_REASON_WINDOW_OVERFLOW
COUNTED = abi.LC_FLAG_COUNTED_CLASSES if hasattr(abi, "LC_FLAG_COUNTED_CLASSES") else None


def crashy(rng, n_ops, p_info, fs, p_perturb=0.5):
    """A 2-valued version-less register, optionally with one CAS class;
    crashed writes take effect with p = 0.5."""
    val, recs, infos = N, [], []
    for _ in range(n_ops):
        f = rng.choice(fs)
        if f == R:
            recs.append([R, val, N, N]); infos.append(False)
        elif f == W:
            v = rng.randrange(2); info = rng.random() < p_info
            if not info or rng.random() < 0.5: val = v
            recs.append([W, v, N, N]); infos.append(info)
        else:
            info = rng.random() < p_info; ok = val == 0
            if not ok and not info: continue
            if ok and (not info or rng.random() < 0.5): val = 1
            recs.append([C, 1, 0, N]); infos.append(info)
    out = [r + list(t) for r, t in zip(recs, _intervals(rng, len(recs), infos, 25))]
    out.sort(key=lambda r: r[4])
    reads = [i for i, r in enumerate(out) if r[0] == R and r[1] != N]
    if reads and rng.random() < p_perturb:
        j = rng.choice(reads); out[j][1] = rng.choice([1 - out[j][1], 2])
    return out


@functools.lru_cache(maxsize=None)
def batch(name):
    """(keys, init_value) of the batches A-D."""
    if name == "A":
        rng = random.Random(0xCC11)
        return [crashy(rng, rng.randrange(700, 1000), 0.35, [R, R, W]) for _ in range(24)], N
    if name == "B":
        rng = random.Random(0xCC12)
        return [crashy(rng, rng.randrange(500, 700), 0.30, [R, R, R, W, C]) for _ in range(8)], N
    if name == "C":
        rng = random.Random(0xC1A59)
        return [random_mutex(rng, rng.randrange(200, 800), p_info=0.4, p_perturb=0.5)
                for _ in range(16)], FREE
    rng = random.Random(0xCC14)
    return [random_casreg(rng, rng.randrange(150, 220), p_info=0.6, p_perturb=0.3, n_values=5)
            for _ in range(8)], N


@functools.lru_cache(maxsize=None)
def packed(name):
    keys, init = batch(name)
    ops, off = pack_keys(keys)
    return ops, off, init


@functools.lru_cache(maxsize=None)
def jitc(name):
    """The oracle's JITC results of a batch: computed once, never modified."""
    ops, off, init = packed(name)
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8, max_configs=1 << 22,
                        init_value=init)
    j.setflags(write=False)
    return j


def opts(name, flags=0, **kw):
    return abi.default_opts(init_value=packed(name)[2], flags=flags, **kw)


def assert_equal(got, ref, what, keys=None):
    for k in (range(len(ref)) if keys is None else keys):
        for f in FIELDS:
            assert int(got[f][k]) == int(ref[f][k]), (what, k, f, int(got[f][k]), int(ref[f][k]))


# ------------------------------------------------------------------ CPU tests

def test_symbols():
    assert abi.LC_FLAG_COUNTED_CLASSES == 32
    L = abi.lib()
    assert L.lc_counted_plan is not None and L.lc_last_counted_stats is not None
    assert L.lc_abi_version() == 5


def layout_ref(recs):
    """The layout rule (include/lincheck.h, lc_counted_plan), restated."""
    members = {}  # (dicts keep insertion order: first call)
    for r in recs:
        if r[0] in (W, C) and r[5] == INF:
            members[tuple(r[:4])] = members.get(tuple(r[:4]), 0) + 1
    classes, bits = [], 0
    for (f, v, e, ver), m in members.items():
        width = m.bit_length()  # floor(log2 m) + 1
        bits += width
        classes.append({"f": f, "value": v, "expected": e, "version": ver, "members": m,
                        "shift": 64 - bits, "width": width})
    slots = min(64 - bits, 64 - len(classes))
    return {"n_classes": len(classes), "field_bits": bits, "slots": slots,
            "fits": int(len(classes) <= 16 and slots >= 1), "classes": classes[:16]}


def _crashed_writes(sizes, t0=0):
    """Crashed writes of value c, sizes[c] of them, classes interleaved."""
    recs, t = [], t0
    left = list(sizes)
    while any(left):
        for c, m in enumerate(left):
            if m:
                recs.append([W, c, N, N, t, INF])
                left[c] -= 1
                t += 1
    return recs


def _layout_cases():
    cases = {}
    for name in "ABCD":
        for i, k in enumerate(batch(name)[0]):
            cases["%s%d" % (name, i)] = k
    cases["no-crash"] = [[W, 1, N, N, 0, 3], [R, 1, N, N, 1, 2], [R, N, N, N, 4, INF]]
    cases["empty"] = []
    cases["widths"] = _crashed_writes([1, 2, 3, 4, 7, 8, 255, 256])
    cases["16-classes"] = _crashed_writes([3] * 16) + [[R, 2, N, N, 100, 101]]
    cases["17-classes"] = _crashed_writes([3] * 17)
    cases["no-slot"] = _crashed_writes([8] * 16)  # 16 x 4 bits: fields fill the mask
    # a crashed write that carries a version is a class of its own, and so
    # is a crashed CAS against a write of the same value
    cases["versioned"] = [[W, 1, N, N, 0, INF], [W, 1, N, 5, 1, INF], [C, 1, 0, N, 2, INF],
                          [W, 1, N, N, 3, INF], [W, 1, N, 5, 4, INF], [W, 1, N, 6, 5, INF],
                          [R, 1, N, N, 6, INF], [W, 1, N, N, 7, 8]]
    return cases


def test_layout_rule():
    cases = _layout_cases()
    for name, recs in cases.items():
        got = abi.counted_plan(np.array(recs, dtype=np.int64).reshape(-1, 6))
        assert got == layout_ref(recs), name
    # what the cases are there for
    assert layout_ref(cases["no-crash"])["n_classes"] == 0
    assert layout_ref(cases["no-crash"])["slots"] == 64
    assert [c["width"] for c in layout_ref(cases["widths"])["classes"]] == [1, 2, 2, 3, 3, 4, 8, 9]
    assert layout_ref(cases["16-classes"])["fits"] == 1
    assert layout_ref(cases["17-classes"])["fits"] == 0
    assert layout_ref(cases["no-slot"])["fits"] == 0
    assert layout_ref(cases["versioned"])["n_classes"] == 4
    assert all(layout_ref(k)["fits"] for n in "ABC" for k in batch(n)[0])
    assert not any(layout_ref(k)["fits"] for k in batch("D")[0])
    crashed = [sum(1 for r in k if r[0] != R and r[5] == INF) for k in batch("A")[0]]
    assert min(crashed) >= 73


def test_counted_plan_rejects_bad_arguments():
    import ctypes
    lay = abi.LcCountedLayout()
    assert abi.lib().lc_counted_plan(None, 3, ctypes.byref(lay)) == -22
    assert abi.lib().lc_counted_plan(None, 0, None) == -22
    assert abi.lib().lc_counted_plan(None, 0, ctypes.byref(lay)) == 0 and lay.slots == 64


def test_checker_passes_the_flag():
    from jepsen.etcd_amd import checker
    import inspect
    assert "counted_classes" in inspect.signature(checker.RegisterChecker.__init__).parameters


# ------------------------------------------------------------------ GPU tests

def _overflowed(ctx, name, flags=0):
    ops, off, _ = packed(name)
    _, plain = ctx.check(ops, off, opts(name, flags))
    return plain, int((plain["reason"] == OVERFLOW).sum())


@pytest.mark.gpu
def test_batch_a_equals_jitc():
    ops, off, _ = packed("A")
    j = jitc("A")
    assert (j["verdict"] != -1).all()
    with abi.Context(1) as ctx:
        plain, n_over = _overflowed(ctx, "A")
        assert ctx.counted_stats()["n_keys"] == 0  # flag off: the tier did not run
        assert n_over >= len(j) // 2
        _, got = ctx.check(ops, off, opts("A", COUNTED))
        st = ctx.counted_stats()
    assert_equal(got, j, "A")
    assert st["n_keys"] == n_over and st["n_decided"] == st["n_keys"] and st["n_unfit"] == 0
    assert st["kernel_ms"] > 0


@pytest.mark.gpu
def test_batch_b_cas_class_equals_jitc():
    ops, off, _ = packed("B")
    j = jitc("B")
    assert (j["verdict"] != -1).all()
    with abi.Context(1) as ctx:
        _, got = ctx.check(ops, off, opts("B", COUNTED))
        assert ctx.counted_stats()["n_keys"] >= 1
    assert_equal(got, j, "B")


@pytest.mark.gpu
def test_legality_per_state_gives_the_same_results(monkeypatch):
    """LC_COUNTED_BY_VALUE=0: legality tested per distinct (version, value)
    of a batch's states, as it is where a pending op constrains the version,
    instead of per distinct value."""
    monkeypatch.setenv("LC_COUNTED_BY_VALUE", "0")
    ops, off, _ = packed("B")
    with abi.Context(1) as ctx:
        _, got = ctx.check(ops, off, opts("B", COUNTED))
        assert ctx.counted_stats()["n_keys"] >= 1
    assert_equal(got, jitc("B"), "B, legality per state")


@pytest.mark.gpu
def test_batch_c_single_configuration_and_65_crashed_writes():
    ops, off, _ = packed("C")
    j = jitc("C")
    with abi.Context(1) as ctx:
        _, got = ctx.check(ops, off, opts("C", COUNTED))
        st = ctx.counted_stats()
        assert st["n_keys"] >= 8 and st["n_decided"] == st["n_keys"]
        assert_equal(got, j, "C")
        # tests/test_gpu.py test_window_overflow_is_unknown's key
        recs = [[1, i % 4, -1, -1, i, INF] for i in range(65)]
        ops, off = pack_keys([recs, [[1, 1, -1, 1, 0, 1]]])
        fl = abi.LC_FLAG_NO_GAP_TIER
        _, plain = ctx.check(ops, off, abi.default_opts(flags=fl))
        assert plain["verdict"][0] == -1 and plain["reason"][0] == OVERFLOW
        _, got = ctx.check(ops, off, abi.default_opts(flags=fl | COUNTED))
        assert ctx.counted_stats()["n_keys"] == 1
    _, j = oracle.check(ops, off, algo=oracle.JITC)
    assert_equal(got, j, "65 crashed writes", [0])  # (key 1: the version-order tier's)
    assert got["verdict"][0] == 1 and got["verdict"][1] == 1


@pytest.mark.gpu
def test_batch_d_does_not_fit_and_stays_as_it_was():
    ops, off, _ = packed("D")
    with abi.Context(1) as ctx:
        plain, n_over = _overflowed(ctx, "D")
        _, got = ctx.check(ops, off, opts("D", COUNTED))
        st = ctx.counted_stats()
        assert_equal(got, plain, "D")
        assert st["n_keys"] == n_over and st["n_unfit"] == n_over and st["n_decided"] == 0
        # keys that do overflow the tiers' window and stay so: 17 classes (no
        # layout), and 66 :ok writes open at once (more than the 64 slots)
        many = _crashed_writes([4] * 17)
        wide = [[W, i, N, N, i, 100 + i] for i in range(66)]
        ops, off = pack_keys([many, wide])
        fl = abi.LC_FLAG_NO_GAP_TIER
        _, plain = ctx.check(ops, off, abi.default_opts(flags=fl))
        assert (plain["reason"] == OVERFLOW).all()
        _, got = ctx.check(ops, off, abi.default_opts(flags=fl | COUNTED))
        st = ctx.counted_stats()
    assert_equal(got, plain, "unfit keys")
    assert st["n_keys"] == 2 and st["n_unfit"] == 2 and st["n_decided"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", [("info", abi.LC_FLAG_NO_GAP_TIER), ("c5", 0)])
def test_flag_is_inert_elsewhere(name, flags):
    import os
    from helpers import GOLDEN
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    with abi.Context(1) as ctx:
        _, a = ctx.check(z["ops"], z["key_off"], abi.default_opts(flags=flags))
        _, b = ctx.check(z["ops"], z["key_off"], abi.default_opts(flags=flags | COUNTED))
        st = ctx.counted_stats()
    assert_equal(b, a, name)
    assert st["n_keys"] == int((a["reason"] == OVERFLOW).sum())


@pytest.mark.gpu
def test_budgets():
    ops, off, _ = packed("A")
    j = jitc("A")
    with abi.Context(1) as ctx:
        _, got = ctx.check(ops, off, opts("A", COUNTED, max_configs_per_key=5000))
        within = [k for k in range(len(j)) if j["configs_explored"][k] <= 5000]
        beyond = [k for k in range(len(j)) if j["configs_explored"][k] > 5000]
        assert within and beyond
        assert_equal(got, j, "A within the budget", within)
        for k in beyond:
            assert (got["verdict"][k], got["reason"][k]) == (-1, abi.LC_REASON_CONFIG_BUDGET), k
        ops, off, _ = packed("B")
        j = jitc("B")
        _, got = ctx.check(ops, off, opts("B", COUNTED, time_budget_ms=1))
    timed_out = [k for k in range(len(j)) if got["reason"][k] == 7]  # LC_REASON_TIME_BUDGET
    assert len(timed_out) >= 1
    for k in range(len(j)):
        if got["verdict"][k] != -1:
            assert_equal(got, j, "B within the time budget", [k])


@pytest.mark.gpu
def test_device_resident_records():
    import torch
    ops, off, _ = packed("A")
    n = len(off) - 1
    dev = torch.device("cuda:0")
    d_ops = torch.from_numpy(ops).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_out = torch.zeros(n * abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    with abi.Context(1) as ctx:
        _, host = ctx.check(ops, off, opts("A", COUNTED))
        host_keys = ctx.counted_stats()["n_keys"]
        ctx.check_device(d_ops.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(),
                         opts=opts("A", COUNTED))
        torch.cuda.synchronize()
        st = ctx.counted_stats()
    got = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=abi.RESULT_DTYPE)
    assert_equal(got, host, "device entry point")
    assert_equal(got, jitc("A"), "device entry point against JITC")
    assert st["n_keys"] == host_keys and st["n_decided"] == host_keys


@pytest.mark.gpu
def test_two_device_contexts_on_one_gpu(monkeypatch):
    monkeypatch.setenv("LC_VIRTUAL_DEVICES", "2")
    ops, off, _ = packed("A")
    with abi.Context(1) as ctx:
        plain, n_over = _overflowed(ctx, "A")
        assert ctx.stats()["n_devices"] == 2
        _, got = ctx.check(ops, off, opts("A", COUNTED))
        st = ctx.counted_stats()
        shares = [d["key_end"] - d["key_begin"] for d in ctx.device_stats()]
    assert min(shares) >= 1  # both devices had keys
    assert_equal(got, jitc("A"), "two device contexts")
    assert st["n_keys"] == n_over and st["n_decided"] == n_over


@pytest.mark.gpu
def test_counted_tier_runs_before_the_whole_gpu_search():
    ops, off, _ = packed("A")
    with abi.Context(1) as ctx:
        _, got = ctx.check(ops, off, opts("A", COUNTED | abi.LC_FLAG_WHOLE_GPU))
        st = ctx.counted_stats()
    assert_equal(got, jitc("A"), "both flags")
    assert st["n_keys"] >= 12 and st["n_decided"] == st["n_keys"]
