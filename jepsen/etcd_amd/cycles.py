"""Batched backward reachability, first hit (include/lincheck_cycles.h): the
primitive behind the Elle checkers' device search for the txn that closes a
G-single cycle.

`cycle_reach(n_nodes, pred_off, pred, q_node, q_head_off, q_heads)` takes a
graph as its predecessor lists (a CSR: int64 offsets, int32 nodes) and queries
ascending by source node, each with a list of heads; query q hits iff one of
its heads reaches q_node[q].  It returns `(hit, summary)`: with
`all_queries=True` hit has one 0 / 1 per query, otherwise it is None and only
the summary's `first_hit` (the least hitting query, or -1) is decided.
"""
from . import abi

ALL = abi.LC_REACH_ALL


def available():
    """Whether the loaded library has the primitive (a LINCHECK_LIB may lack it)."""
    return hasattr(abi.lib(), "lc_cycle_reach")


def cycle_reach(n_nodes, pred_off, pred, q_node, q_head_off, q_heads, all_queries=False, device=True, ctx=None):
    """The search on the device (ctx: an abi.Context, or None for one opened
    for this call on the first GPU) or, with device=False, on the host."""
    args = (n_nodes, pred_off, pred, q_node, q_head_off, q_heads, all_queries)
    if not device:
        return abi.cycle_reach_host(*args)
    if ctx is not None:
        return ctx.cycle_reach(*args)
    with abi.Context(device_mask=1) as c:
        return c.cycle_reach(*args)


def limits():
    """lc_cycle_reach_limits: {"max_nodes", "min_work", "default_min_work", "max_workgroups"}."""
    return abi.cycle_reach_limits()
