"""LC_FLAG_SEARCH_WITNESS: linearization witnesses for the keys the search
tiers decide (witness kinds LC_WITNESS_ORDER_FULL / LC_WITNESS_ORDER_PREFIX,
include/lincheck.h; the device search: csrc/witness_search.hip).

Every order the device returns is certified from the records alone by
tests/order_ref.py (oracle.brute.step plus the real-time rule), which is
itself compared with the product-side check jepsen/etcd_amd/witness.py; the
CPU tests pin the two certifiers against orders found by exhaustive search
and against tampered orders."""
import functools
import os
import random
import re

import numpy as np
import pytest

import order_ref
from helpers import FREE, GOLDEN, HELD, INF, C, N, R, W, pack_keys, random_casreg, random_mutex, \
    random_tiny
from jepsen.etcd_amd import abi, checker, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SW = getattr(abi, "LC_FLAG_SEARCH_WITNESS", None)
FULL, PREFIX = 3, 4
MODELS = {"mutex": (random_mutex, FREE, 0), "cas-register": (random_casreg, N, 0),
          "register": (random_tiny, N, abi.LC_FLAG_NO_FAST_PATH)}


def both(recs, w, kind, cut, init):
    """The two certifiers' answer (they must agree)."""
    a = order_ref.certify(recs, w, cut if kind == PREFIX else None, (0, init))
    b = witness.certify(recs, w, kind, cut, (0, init))
    assert a == b, (recs, list(w), kind, cut)
    return a


@functools.lru_cache(maxsize=None)
def tiny_keys(model, n_keys, max_ops, seed):
    gen = MODELS[model][0]
    rng = random.Random(seed)
    return tuple(tuple(map(tuple, gen(rng, rng.randrange(0, max_ops + 1)))) for _ in range(n_keys))


@functools.lru_cache(maxsize=None)
def searched(model):
    """300 tiny keys of a model with what the exhaustive search says: per key
    (records, kind, cut, witness) — the whole history when it has an order,
    else the prefix before the first return whose prefix has none."""
    out = []
    init = MODELS[model][1]
    for recs in tiny_keys(model, 300, 7, 0x5117):
        w = order_ref.find_order(recs, None, (0, init))
        if w is not None:
            out.append((recs, FULL, None, tuple(w)))
            continue
        for ret in sorted(r[5] for r in recs if r[5] != INF):
            if order_ref.find_order(recs, ret, (0, init)) is None:
                w = order_ref.find_order(recs, ret - 1, (0, init))
                assert w is not None  # (the earlier returns' prefixes had orders)
                out.append((recs, PREFIX, ret - 1, tuple(w)))
                break
        else:
            raise AssertionError("no whole order, yet every return's prefix has one")
    return out


# ------------------------------------------------------------------ CPU tests

def test_symbols_and_constants():
    L = abi.lib()
    assert L.lc_last_witness_stats is not None  # (the feature's marker)
    assert L.lc_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "lincheck.h")).read()
    for name in ("LC_FLAG_SEARCH_WITNESS", "LC_WITNESS_ORDER_FULL", "LC_WITNESS_ORDER_PREFIX"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(abi, name), name
    assert (abi.LC_FLAG_SEARCH_WITNESS, abi.LC_WITNESS_ORDER_FULL, abi.LC_WITNESS_ORDER_PREFIX) == \
        (64, FULL, PREFIX)
    assert (witness.LC_WITNESS_ORDER_FULL, witness.LC_WITNESS_ORDER_PREFIX) == (FULL, PREFIX)
    hdr = open(os.path.join(ROOT, "include", "lincheck_witness.h")).read()
    fields = re.search(r"typedef struct lc_witness_stats \{(.*?)\} lc_witness_stats;", hdr, re.S).group(1)
    assert re.findall(r"(?:int64_t|double)\s+(\w+);", fields) == [f for f, _ in abi.LcWitnessStats._fields_]


def test_exhaustive_search_agrees_with_brute():
    from oracle import brute
    for model in MODELS:
        init = MODELS[model][1]
        for recs in tiny_keys(model, 120, 5, 0xB07E):
            assert (order_ref.find_order(recs, None, (0, init)) is not None) == \
                brute.check(list(recs), (0, init)), recs


@pytest.mark.parametrize("model", list(MODELS))
def test_certifiers_accept_searched_orders(model):
    kinds = set()
    for recs, kind, cut, w in searched(model):
        assert both(recs, w, kind, cut, MODELS[model][1]), (recs, w, kind, cut)
        kinds.add(kind)
        assert witness.order(recs, w) == sorted((i for i in range(len(w)) if w[i] >= 0),
                                                key=lambda i: w[i])
    assert kinds == {FULL, PREFIX}


@pytest.mark.parametrize("model", list(MODELS))
def test_certifiers_reject_tampered_orders(model):
    init = MODELS[model][1]
    n = {"swap": 0, "drop": 0, "dup": 0, "late": 0}
    for recs, kind, cut, w in searched(model):
        ranked = [i for i in range(len(w)) if w[i] >= 0]
        # two ranks swapped across a real-time edge
        edge = [(a, b) for a in ranked for b in ranked if recs[a][5] < recs[b][4]]
        if edge:
            a, b = edge[0]
            t = list(w)
            t[a], t[b] = t[b], t[a]
            assert not both(recs, t, kind, cut, init)
            n["swap"] += 1
        # an :ok op (one the cut requires) dropped, the ranks closed up
        req = [i for i in ranked if recs[i][5] <= (cut if kind == PREFIX else INF - 1)]
        if req:
            t = [-1 if i == req[0] else x - (x > w[req[0]]) for i, x in enumerate(w)]
            assert not both(recs, t, kind, cut, init)
            n["drop"] += 1
        # a rank used twice
        if len(ranked) >= 2:
            t = list(w)
            t[ranked[0]] = t[ranked[1]]
            assert not both(recs, t, kind, cut, init)
            n["dup"] += 1
        # an op called after the cut, ranked last
        late = [i for i in range(len(w)) if kind == PREFIX and recs[i][4] > cut]
        if late:
            t = list(w)
            t[late[0]] = len(ranked)
            assert not both(recs, t, kind, cut, init)
            n["late"] += 1
    assert min(n.values()) > 0, n


def test_certifiers_reject_model_violations():
    # a read of a value nobody wrote; a CAS from the wrong value; a version skipped
    for recs in ([[W, 1, N, N, 0, 1], [R, 2, N, N, 2, 3]],
                 [[W, 1, N, N, 0, 1], [C, 2, 0, N, 2, 3]],
                 [[W, 1, N, 1, 0, 1], [W, 2, N, 3, 2, 3]]):
        assert not both(recs, [0, 1], FULL, None, N)
        assert both(recs, [0, -1], PREFIX, 1, N)
    # the wrong kind / a missing cut / a witness of the wrong length
    recs = [[W, 1, N, N, 0, 1]]
    assert witness.certify(recs, [0], FULL) and not witness.certify(recs, [0], PREFIX)
    assert not witness.certify(recs, [0], 1) and not witness.certify(recs, [0, 1], FULL)
    assert not order_ref.certify(recs, [0, 1])


# ------------------------------------------------------------------ GPU tests

class Run:
    """A batch checked without and with the flag (both with lc_aux): res /
    wit / kind / st with the flag, wit0 / kind0 without."""


def run(ctx, keys, init, flags=0, **kw):
    """The results with the flag must equal the ones without, field for
    field, and so must the kinds and witnesses the tiers themselves gave."""
    r = Run()
    r.init = init
    r.ops, r.off = pack_keys([list(map(list, k)) for k in keys])
    _, plain, r.wit0, r.kind0 = ctx.check(r.ops, r.off, abi.default_opts(init_value=init, flags=flags, **kw),
                                          witness=True)
    assert ((r.kind0 >= 0) & (r.kind0 <= 2)).all()  # (the new kinds never come unasked)
    _, r.res, r.wit, r.kind = ctx.check(r.ops, r.off,
                                        abi.default_opts(init_value=init, flags=flags | SW, **kw),
                                        witness=True)
    r.st = ctx.last_witness_stats()
    assert r.res.tobytes() == plain.tobytes()
    return r


def certify_all(r, want_all=True):
    """A key the tiers witnessed keeps its kind and witness, byte for byte.
    Every ORDER kind sits on a decided key of the matching verdict and is
    certified at its cut; with want_all every other decided key has one.
    Returns the number of ORDER witnesses."""
    n = 0
    off = r.off
    for k in range(len(r.res)):
        v, kind = int(r.res["verdict"][k]), int(r.kind[k])
        if r.kind0[k] != 0:
            assert kind == r.kind0[k], k
            assert r.wit[off[k]:off[k + 1]].tobytes() == r.wit0[off[k]:off[k + 1]].tobytes(), k
            continue
        if want_all and v in (0, 1):
            assert kind == (FULL if v == 1 else PREFIX), (k, v, kind)
        if kind in (FULL, PREFIX):
            assert v == (1 if kind == FULL else 0), k
            recs, w = r.ops[off[k]:off[k + 1]], r.wit[off[k]:off[k + 1]]
            assert both(recs, w, kind, int(r.res["fail_prefix_end"][k]) - 1, r.init), \
                (k, recs.tolist(), w.tolist())
            n += 1
        else:
            assert kind == 0, (k, kind)
    return n


@pytest.mark.gpu
def test_hand_cases(ctx):
    """* A 5-op mutex key (a crashed acquire that has to take effect: the
      second release needs it).  In a mutex history every legal candidate at a
      node is of one class (all acquires, or all releases), so trying the
      returning op, then the earliest deadline, never meets a dead end
      (exchange argument; a Python restatement of the search backtracked on
      none of 19,000 random mutex keys): this order is found in 5 steps.
    * A 5-op cas-register key whose first candidate IS a dead end: the write
      that returns first has to come after the CAS from nil, so the search
      backtracks and stores dead ends (more steps than ops ranked).
    * One op."""
    mutex = [[C, HELD, FREE, N, 0, INF], [C, HELD, FREE, N, 1, 4], [C, FREE, HELD, N, 2, 3],
             [C, FREE, HELD, N, 5, 6], [C, HELD, FREE, N, 7, 8]]
    r = run(ctx, [mutex], FREE)
    assert r.res["verdict"][0] == 1 and certify_all(r) == 1
    assert (r.wit >= 0).all() and r.st["n_found"] == 1 and r.st["nodes"] == 5
    casreg = [[W, 0, N, N, 0, 3], [C, 2, N, N, 1, 5], [W, 1, N, N, 2, 6], [C, 0, 1, N, 4, 8],
              [R, 0, N, N, 7, 9]]
    r = run(ctx, [casreg], N)
    assert r.res["verdict"][0] == 1 and certify_all(r) == 1
    assert r.st["nodes"] > int((r.wit >= 0).sum()) == 5, r.st
    r = run(ctx, [[[W, 1, N, N, 0, 1]]], N)
    assert r.kind.tolist() == [FULL] and r.wit.tolist() == [0] and r.st["nodes"] == 1


@pytest.mark.gpu
def test_ops_open_across_the_chunk_boundary(ctx):
    """A cas-register key of 70 records whose 65th record is called while
    earlier ops (a crashed one among them) are still open."""
    for seed in range(1000):
        rng = random.Random(seed)
        recs = random_casreg(rng, 85, p_info=0.1, p_perturb=0.0)
        if len(recs) != 70:
            continue
        t = recs[64][4]
        if sum(1 for x in recs[:64] if x[5] > t) >= 3 and any(x[5] == INF for x in recs[:60]):
            break
    else:
        raise AssertionError("no 70-record key with ops open across the boundary")
    r = run(ctx, [recs], N)
    assert r.res["verdict"][0] == 1 and certify_all(r) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(MODELS))
def test_random_tiny_keys(ctx, model):
    _, init, flags = MODELS[model]
    keys = tiny_keys(model, 600, 12, 0x7191)
    r = run(ctx, keys, init, flags)
    res = r.res
    # keys for the search: decided, and not witnessed by the tiers already
    # (kinds 1 and 2, which certify_all wants unchanged: empty keys for one)
    todo = int(((res["verdict"] != -1) & (r.kind0 == 0)).sum())
    assert todo > 400 and 30 < int((res["verdict"] == 0).sum()) < 570
    if flags & abi.LC_FLAG_NO_FAST_PATH:
        assert (r.kind0 == 0).all()
    assert certify_all(r) == todo
    assert (r.st["n_keys"], r.st["n_found"], r.st["n_budget"], r.st["n_window"]) == (todo, todo, 0, 0)
    for k, recs in enumerate(keys):  # the verdict itself, by exhaustive search
        if len(recs) <= 8 and res["verdict"][k] != -1:
            whole = order_ref.find_order(recs, None, (0, init)) is not None
            assert whole == (res["verdict"][k] == 1), k
            if not whole:
                end = int(res["fail_prefix_end"][k])
                assert order_ref.find_order(recs, end, (0, init)) is None, k


@pytest.mark.gpu
def test_synthetic_cas_register_keys(ctx):
    """200 keys x 200 ops at concurrency 10, versions stripped (the batch shape
    of tools/frontier_dist.py): every decided key witnessed within the default
    budget."""
    ops, off, _, _ = abi.synth(200, 200, concurrency=10, p_anomaly=0.2, seed=0x5EED0009)
    ops = ops.copy()
    ops[:, 3] = -1
    keys = [ops[off[k]:off[k + 1]].tolist() for k in range(200)]
    r = run(ctx, keys, N)
    print("synthetic 200 x 200:", r.st)
    assert (r.kind0 == 0).all() and (r.res["verdict"] != -1).all()
    assert 0 < int((r.res["verdict"] == 0).sum()) < 200
    assert certify_all(r) == 200
    assert r.st["n_found"] == r.st["n_keys"] == 200 and r.st["n_budget"] == r.st["n_window"] == 0


@pytest.mark.gpu
def test_versioned_keys_keep_their_witnesses(ctx):
    """C5: kinds 1 and 2 and their witnesses are byte-identical with the flag
    (certify_all), and the keys a search decided gain an order."""
    z = np.load(os.path.join(GOLDEN, "c5.npz"))
    off = z["key_off"]
    r = run(ctx, [z["ops"][off[k]:off[k + 1]].tolist() for k in range(len(off) - 1)], N)
    assert int(((r.kind0 == 1) | (r.kind0 == 2)).sum()) > 250
    certify_all(r)


@pytest.mark.gpu
def test_window_overflow(ctx):
    """70 crashed acquires stay open: the counted tier decides the key, the
    witness search (one slot per open op) leaves it alone."""
    recs = [[C, HELD, FREE, N, t, INF] for t in range(70)]
    recs += [[C, HELD, FREE, N, 70, 71], [C, FREE, HELD, N, 72, 73], [C, FREE, HELD, N, 74, 75]]
    r = run(ctx, [recs], FREE, abi.LC_FLAG_COUNTED_CLASSES)
    assert r.res["verdict"][0] == 1
    assert r.kind.tolist() == [0] and r.wit.tobytes() == r.wit0.tobytes()
    assert (r.st["n_keys"], r.st["n_found"], r.st["n_budget"], r.st["n_window"]) == (1, 0, 0, 1)


@pytest.mark.gpu
def test_budget(ctx):
    """max_configs_per_key bounds the witness search's steps too: the frontier
    search takes the reads of a write-then-30-reads key in its read closure (2
    configurations explored), yet ranking the 31 ops takes 31 steps."""
    seq = [[W, 1, N, N, 0, 1]] + [[R, 1, N, N, 2 * i, 2 * i + 1] for i in range(1, 31)]
    keys = [seq] * 8 + [seq[:4]] * 8
    r = run(ctx, keys, N, max_configs_per_key=8)
    print("budget 8: configs_explored", r.res["configs_explored"].tolist(), r.st)
    decided = r.res["verdict"] != -1
    assert decided[8:].all()
    certify_all(r, want_all=False)
    assert (r.kind[8:] == FULL).all() and (r.kind[:8] == 0).all()
    assert r.st["n_budget"] == int(decided[:8].sum()) >= 1
    assert r.st["n_found"] == 8 and r.st["n_keys"] == r.st["n_found"] + r.st["n_budget"]
    # under a time budget the call still returns 0 and counts every key
    r = run(ctx, keys, N, time_budget_ms=1)
    certify_all(r, want_all=False)
    assert r.st["n_keys"] == r.st["n_found"] + r.st["n_budget"] == int((r.res["verdict"] != -1).sum())


@pytest.mark.gpu
def test_device_resident(ctx):
    import torch
    r = run(ctx, tiny_keys("cas-register", 600, 12, 0x7191), N)
    dev = torch.device("cuda:0")
    n = len(r.off) - 1
    d_ops, d_off = torch.from_numpy(r.ops).to(dev), torch.from_numpy(r.off).to(dev)
    d_out = torch.zeros(n * abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_wit = torch.full((len(r.ops),), -3, dtype=torch.int32, device=dev)
    d_kind = torch.full((n,), -3, dtype=torch.int32, device=dev)
    ctx.check_device(d_ops.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(),
                     opts=abi.default_opts(flags=SW), d_witness=d_wit.data_ptr(),
                     d_witness_kind=d_kind.data_ptr())
    torch.cuda.synchronize()
    st2 = ctx.last_witness_stats()
    assert d_out.cpu().numpy().tobytes() == r.res.tobytes()
    assert (d_kind.cpu().numpy() == r.kind).all() and (d_wit.cpu().numpy() == r.wit).all()
    assert (st2["n_keys"], st2["n_found"]) == (r.st["n_keys"], r.st["n_found"]) and st2["n_keys"] > 400


@pytest.mark.gpu
def test_two_device_contexts_on_one_gpu(ctx, monkeypatch):
    keys = tiny_keys("cas-register", 600, 12, 0x7191)
    one = run(ctx, keys, N)
    monkeypatch.setenv("LC_VIRTUAL_DEVICES", "2")
    with abi.Context(1) as two_ctx:
        two = run(two_ctx, keys, N)
        assert two_ctx.stats()["n_devices"] == 2
        shares = [d["key_end"] - d["key_begin"] for d in two_ctx.device_stats()]
    assert min(shares) >= 1
    assert two.res.tobytes() == one.res.tobytes() and (two.kind == one.kind).all()
    for a, b in zip(np.cumsum([0] + shares)[:-1], np.cumsum(shares)):  # both ranges witnessed
        assert (two.kind[a:b] >= FULL).sum() > 0
    assert certify_all(two) == one.st["n_found"]
    assert (two.st["n_keys"], two.st["n_found"]) == (one.st["n_keys"], one.st["n_found"])


@pytest.mark.gpu
def test_checker():
    from test_models import MUTEX_KATS, ops_of
    cs = [checker.linearizable(checker.Mutex(), device_mask=1),
          checker.linearizable(checker.Mutex(), device_mask=1, search_witness=False),
          checker.linearizable(checker.Mutex(), device_mask=1, search_witness=True)]
    try:
        for name, seq, valid in MUTEX_KATS:
            plain, off, on = (c.check({}, ops_of(seq)) for c in cs)
            assert off == plain and "linearization" not in plain, name
            assert on["valid?"] is valid and on["witness-certified"] is True, (name, on)
            lin = on["linearization"]
            assert all(op["f"] in ("acquire", "release") for op in lin)
            n_ok = sum(1 for op in ops_of(seq) if op["type"] == "ok")
            if valid:
                assert sum(1 for op in lin if op["type"] == "ok") == n_ok, name
            else:
                assert len(lin) < n_ok and (not lin or on["last-op"] == lin[-1]), name
            extra = {"linearization", "witness-certified", "last-op"}
            assert {k: v for k, v in on.items() if k not in extra} == \
                {k: v for k, v in plain.items() if k not in extra}, name
    finally:
        for c in cs:
            c.close()
