"""The reference for lc_cycle_reach (include/lincheck_cycles.h), written
plainly: a breadth-first search per query over Python lists."""


def reach(n_nodes, pred_off, pred, q_node, q_head_off, q_heads):
    """-> (hit, one 0 / 1 per query; first_hit; the nodes the searches mark, each run to exhaustion)."""
    hit, visited = [], 0
    for q, src in enumerate(q_node):
        heads = set(int(h) for h in q_heads[q_head_off[q]:q_head_off[q + 1]])
        seen, queue = {int(src)}, [int(src)]
        for b in queue:
            for a in pred[pred_off[b]:pred_off[b + 1]]:
                if int(a) not in seen:
                    seen.add(int(a))
                    queue.append(int(a))
        hit.append(int(bool(heads & (seen - {int(src)}))))
        visited += len(seen)
    return hit, (hit.index(1) if 1 in hit else -1), visited


def first_hit(n_nodes, pred_off, pred, q_node, q_head_off, q_heads):
    return reach(n_nodes, pred_off, pred, q_node, q_head_off, q_heads)[1]


def csr(n_nodes, edges):
    """Predecessor lists of a graph given as (from, to) pairs, in the pairs' order -> (pred_off, pred)."""
    lists = [[] for _ in range(n_nodes)]
    for a, b in edges:
        lists[b].append(a)
    off = [0]
    for ls in lists:
        off.append(off[-1] + len(ls))
    return off, [a for ls in lists for a in ls]


def queries(qs):
    """[(source, [heads])] ascending by source -> (q_node, q_head_off, q_heads)."""
    off = [0]
    for _, hs in qs:
        off.append(off[-1] + len(hs))
    return [s for s, _ in qs], off, [h for _, hs in qs for h in hs]
