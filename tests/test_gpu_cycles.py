"""lc_cycle_reach against lc_cycle_reach_host: with LC_REACH_ALL every hit[q],
first_hit and nodes_visited, then once more without the flag first_hit alone;
on graphs planted at the kernel's edges (bitmap words, the workgroup's width,
the long-list threshold, the launch's workgroup count, max_nodes), on the
KATs and on 100 random graphs."""
import errno

import numpy as np
import pytest

from jepsen.etcd_amd import abi, cycles as CY
from test_cycles import KATS, kat_arrays, random_graph

pytestmark = pytest.mark.gpu

LIM = CY.limits()
MAX_NODES, MAX_WG = LIM["max_nodes"], LIM["max_workgroups"]


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def csr(n, frm, to):
    """Predecessor lists from edge arrays, a node's predecessors in the edges' order."""
    frm, to = np.asarray(frm, np.int64), np.asarray(to, np.int64)
    order = np.argsort(to, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(to, minlength=n), out=off[1:])
    return off, frm[order].astype(np.int32)


def queries(qs):
    qs = sorted(qs)
    off = np.zeros(len(qs) + 1, np.int64)
    off[1:] = np.cumsum([len(h) for _, h in qs])
    heads = np.array([x for _, h in qs for x in h], np.int32)
    return np.array([s for s, _ in qs], np.int32), off, heads


def agree(ctx, n, pred_off, pred, q_node, q_head_off, q_heads, what=""):
    args = (n, pred_off, pred, q_node, q_head_off, q_heads)
    want_hit, want = CY.cycle_reach(*args, all_queries=True, device=False)
    hit, s = ctx.cycle_reach(*args, all_queries=True)
    bad = np.nonzero(hit != want_hit)[0]
    assert len(bad) == 0, (what, bad[:5].tolist(), want_hit[bad[:5]].tolist(), hit[bad[:5]].tolist())
    assert [s[k] for k in ("first_hit", "nodes_visited", "n_queries_run")] == \
        [want[k] for k in ("first_hit", "nodes_visited", "n_queries_run")], (what, s, want)
    none, s = ctx.cycle_reach(*args)
    assert none is None and s["first_hit"] == want["first_hit"], (what, s, want)
    return want["first_hit"], want_hit


def chain(n):
    """i + 1 -> i: node 0 is reached by every node, at depth n - 1 from the last."""
    return csr(n, np.arange(1, n), np.arange(0, n - 1))


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 2047, 2048, 2049))
def test_chains_across_the_bitmap_words(ctx, n):
    """A chain of depth n - 1: the source's last ancestor is the head, in the
    bitmap's last word; every node queried, the hits a prefix."""
    off, pred = chain(n)
    qs = [(i, [n - 1] if i < n - 1 else []) for i in range(n)]
    first, hit = agree(ctx, n, off, pred, *queries(qs), n)
    assert first == (0 if n > 1 else -1) and hit.sum() == n - 1
    # only the first node's query can hit a head that only it descends from: a miss for all the others
    qs = [(i, [j for j in (i - 1,) if j >= 0]) for i in range(n)]
    assert agree(ctx, n, off, pred, *queries(qs), (n, "heads below"))[0] == -1


def test_max_nodes_and_one_more(ctx):
    """A binary heap (the predecessors of i are 2i + 1 and 2i + 2) of
    max_nodes nodes: depth 18, every node visited from the root, the head in
    the bitmaps' last word.  One node more is -E2BIG and writes nothing."""
    for n in (MAX_NODES, MAX_NODES + 1):
        child = np.arange(1, n)
        off, pred = csr(n, child, (child - 1) // 2)
        q = queries([(0, [n - 1]), (1, [n - 1]), (2, [1]), (n - 2, [0])])
        if n == MAX_NODES:
            first, hit = agree(ctx, n, off, pred, *q, "max_nodes")
            assert first == 0 and hit[0] == 1 and hit[2:].tolist() == [0, 0]  # (1 is no descendant of 2; a leaf has none)
        else:
            for all_queries in (True, False):
                with pytest.raises(abi.LcError) as e:
                    ctx.cycle_reach(n, off, pred, *q, all_queries=all_queries)
                assert e.value.code == -errno.E2BIG and (e.value.call.hit == -7).all()
                assert e.value.call.summary.first_hit == 0 and e.value.call.summary.total_ms == 0
            assert CY.cycle_reach(n, off, pred, *q, device=False)[1]["first_hit"] == 0  # (the host has no limit)
    agree(ctx, *kat_arrays(KATS[0]), "after -E2BIG")


@pytest.mark.parametrize("width", (63, 64, 65, 255, 256, 257, 4 * 256 + 1))
def test_one_long_predecessor_list(ctx, width):
    """Node 0 has `width` predecessors (around the long-list threshold, the
    workgroup's width and several of its steps), each with a tail of its own;
    the head hangs below the last of them."""
    n = 2 * width + 2
    frm = np.concatenate([np.arange(1, width + 1), np.arange(width + 1, 2 * width + 1), [2 * width + 1]])
    to = np.concatenate([np.zeros(width, np.int64), np.arange(1, width + 1), [2 * width]])
    off, pred = csr(n, frm, to)
    qs = [(0, [2 * width + 1]), (1, [2 * width + 1]), (width, [2 * width + 1]), (2 * width, [0])]
    first, hit = agree(ctx, n, off, pred, *queries(qs), width)
    assert hit.tolist() == [1, 0, 1, 0]


def test_a_star_and_many_long_lists_in_one_pass(ctx):
    """Every leaf points at the hub and the hub at every leaf: from a leaf the
    first pass has one long list, and 300 hubs in one queue chunk fill the
    window of long lists."""
    n = 1501
    leaves = np.arange(1, n)
    off, pred = csr(n, np.concatenate([leaves, np.zeros(n - 1, np.int64)]), np.concatenate([np.zeros(n - 1, np.int64), leaves]))
    assert agree(ctx, n, off, pred, *queries([(0, [7]), (5, [1500]), (1500, [])]), "star")[1].tolist() == [1, 1, 0]
    hubs, fan = 300, 70  # node 0 <- 300 hubs <- 70 leaves each
    frm = np.concatenate([np.arange(1, hubs + 1), np.arange(hubs + 1, hubs + 1 + hubs * fan)])
    to = np.concatenate([np.zeros(hubs, np.int64), 1 + np.arange(hubs * fan) // fan])
    n = hubs + 1 + hubs * fan
    off, pred = csr(n, frm, to)
    assert agree(ctx, n, off, pred, *queries([(0, [n - 1]), (1, [n - 1]), (hubs, [n - 1])]), "hubs")[1].tolist() == \
        [1, 0, 1]


@pytest.mark.parametrize("n_heads", (0, 1, 64, 65, 300))
def test_head_lists(ctx, n_heads):
    """Head lists around a wave and above the workgroup's width; only the last
    head of the list is an ancestor.  The same list twice in a row, so that
    bits a query left behind would show."""
    n = 800
    off, pred = chain(n)
    rng = np.random.default_rng(n_heads)
    below = rng.permutation(np.arange(0, 400))[:max(n_heads - 1, 0)].tolist()  # descendants: no hit
    qs = [(400, below), (401, below + [799][:n_heads]), (402, below), (403, below + [799][:n_heads]), (404, [])]
    first, hit = agree(ctx, n, off, pred, *queries(qs), n_heads)
    assert hit.tolist() == ([0, 1, 0, 1, 0] if n_heads else [0] * 5)


@pytest.mark.parametrize("n_queries", (0, 1, MAX_WG - 1, MAX_WG, MAX_WG + 1, 3 * MAX_WG + 7))
@pytest.mark.parametrize("hits", ("none", "last", "first-and-last"))
def test_query_counts_around_the_launch(ctx, n_queries, hits):
    """As many queries as the launch starts workgroups, one fewer, one more,
    and several rounds of tickets; the only hit in the last query, or in the
    first and the last."""
    n = 3 * MAX_WG + 10
    assert abi.cycle_reach_limits()["max_workgroups"] == MAX_WG and n * MAX_WG * 4 < (256 << 20)  # (the queues fit)
    off, pred = chain(n)
    qs = []
    for q in range(n_queries):
        hit = hits != "none" and (q == n_queries - 1 or (hits == "first-and-last" and q == 0))
        qs.append((q, [n - 1] if hit else ([q - 1] if q else [])))
    first, _ = agree(ctx, n, off, pred, *queries(qs), (n_queries, hits))
    assert first == (-1 if hits == "none" or not n_queries else n_queries - 1 if hits == "last" else 0)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(ctx, kat):
    first, hit = agree(ctx, *kat_arrays(kat), kat["name"])
    assert (hit.tolist(), first) == (kat["hit"], kat["first_hit"])


def test_random_graphs(ctx):
    firsts = []
    for seed in range(100):
        n, off, pred, qn, qo, qh = random_graph(1000 + seed)
        big = np.random.default_rng(seed)  # and up to 500 nodes
        if seed % 4 == 0:
            n = int(big.integers(300, 501))
            e = big.integers(0, n, (int(big.integers(n, 4 * n)), 2))
            off, pred = csr(n, e[:, 0], e[:, 1])
            qn, qo, qh = queries([(s, [int(h) for h in big.integers(0, n, 3) if h != s]) for s in range(0, n, 2)])
        firsts.append(agree(ctx, n, off, pred, qn, qo, qh, seed)[0])
    assert sum(f == -1 for f in firsts) >= 5 and sum(f >= 0 for f in firsts) >= 20, firsts


def test_einval_writes_nothing_and_the_context_stays_usable(ctx):
    n, off, pred, qn, qo, qh = kat_arrays(KATS[5])
    for bad in ((n, off, pred, qn[::-1], qo, qh), (n, off, [9] + list(pred[1:]), qn, qo, qh),
                (n, off, pred, qn, qo, [1] + list(qh[1:]))):
        for all_queries in (True, False):
            with pytest.raises(abi.LcError) as e:
                ctx.cycle_reach(*bad, all_queries=all_queries)
            assert e.value.code == -errno.EINVAL and "lc_cycle_reach" in str(e.value)
            assert (e.value.call.hit == -7).all() and e.value.call.summary.total_ms == 0
        agree(ctx, n, off, pred, qn, qo, qh, "after -EINVAL")


def test_workspace_reuse(ctx):
    """A large call, a small one, the large one again: the arena only grows,
    and nothing of one call shows in the next."""
    big, small = random_graph(1003), kat_arrays(KATS[1])
    for args in (big, small, big, small):
        agree(ctx, *args, "reuse")
