"""The cycle screen of include/lincheck_screen.h: a transaction graph proved
free of nontrivial SCCs on the device, so that the Elle checkers' host graph
pass can be skipped for the histories that have none.

`cycle_screen(txns, edges)` takes what `lc_append_check` / `lc_wr_check`
return and take: the txn records (abi.AP_TXN_DTYPE, ascending by inv_pos) and
the data edges (abi.AP_EDGE_DTYPE, sorted and unique, both ends nodes).  It
returns `(arrays, summary)`: per txn `reach_lo` (the least completion
reachable), `reach_hi` (the greatest invoke that reaches it) and `mark` (bit 0:
in an SCC with a real-time edge inside; bit 1: survives the trim), and the
summary's `clean` (1: proved acyclic, 0: not proved, -1: gave up after
`max_rounds` rounds), counts, round counts and times.
"""
from . import abi

RT, TRIM = abi.LC_SCREEN_RT, abi.LC_SCREEN_TRIM


def available():
    """Whether the loaded library has the screen (a LINCHECK_LIB may lack it)."""
    return hasattr(abi.lib(), "lc_cycle_screen")


def cycle_screen(txns, edges, device=True, ctx=None):
    """The screen on the device (ctx: an abi.Context, or None for one opened
    for this call on the first GPU) or, with device=False, on the host."""
    if not device:
        return abi.cycle_screen_host(txns, edges)
    if ctx is not None:
        return ctx.cycle_screen(txns, edges)
    with abi.Context(device_mask=1) as c:
        return c.cycle_screen(txns, edges)


def limits():
    """lc_screen_limits: {"max_rounds", "default_max_rounds"}."""
    return abi.screen_limits()
