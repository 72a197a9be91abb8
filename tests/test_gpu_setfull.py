"""lc_set_full on the GPU against lc_set_full_host, bit for bit in every
element record and in every count of the summary: at the word and wave edges
of the bitmap's rows, against the element kernel's stop rule, through table
collisions, tiles, workspace reuse and every error."""
import errno

import numpy as np
import pytest

import setfull_cases as C
import setfull_ref as REF
from jepsen.etcd_amd import abi, setfull as SF
from test_setfull import EINVAL_CASES, GOOD, KATS

pytestmark = pytest.mark.gpu

COUNTS = ("valid", "linearizable", "n_elements", "n_stable", "n_lost", "n_never_read", "n_stale",
          "n_duplicated", "n_phantom")
EDGES_R = (1, 31, 32, 33, 63, 64, 65, 129)
EDGES_E = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def _agree(ctx, adds, reads, values, linearizable=True, what="", tiles=None):
    adds, reads, values = C.arrays(adds, reads, values)
    want, ws = abi.set_full_host(adds, reads, values, linearizable)
    got, gs = ctx.set_full(adds, reads, values, linearizable)
    bad = np.nonzero(want != got)[0]
    assert len(bad) == 0, (what, bad[:5].tolist(), want[bad[:3]].tolist(), got[bad[:3]].tolist())
    assert [gs[k] for k in COUNTS] == [ws[k] for k in COUNTS], (what, gs, ws)
    if tiles is not None:
        assert gs["n_tiles"] == tiles, (what, gs["n_tiles"], tiles)
    return got, gs


def _slot(v, cap):
    """setfull.h's slot_of."""
    m = (1 << 64) - 1
    x = v & m
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & m
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & m
    x ^= x >> 33
    return x & (cap - 1)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(ctx, kat):
    enc = SF.encode(kat["history"])
    got, gs = _agree(ctx, enc.adds, enc.reads, enc.values, kat["linearizable"], kat["name"])
    assert {1: True, 0: False, -1: "unknown"}[gs["valid"]] == kat["valid"]
    assert [REF.OUTCOME_CODE[e["outcome"]] for e in kat["elements"]] == got["outcome"].tolist()


@pytest.mark.parametrize("n_reads", EDGES_R)
def test_word_and_wave_edges(ctx, n_reads):
    for n_elements in EDGES_E:
        for seed in (1, 2):
            _agree(ctx, *C.random_case(seed * 1000 + n_reads, n_elements, n_reads),
                   what=(n_elements, n_reads, seed))


@pytest.mark.parametrize("seen", ("all", "none", "odd"))
def test_suffix_starts_at_every_edge(ctx, seen):
    for first in (0,) + EDGES_R + (130,):
        got, _ = _agree(ctx, *C.ladder(130, first, 3, seen), what=(seen, first))
        # read columns below `first` do not concern the elements
        if seen == "all" and first < 130:
            assert (got["known_pos"] == 10 + 6 * first).all() and (got["last_absent"] == -1).all()
        if seen == "none" or first == 130:
            assert (got["last_present"] == -1).all()


@pytest.mark.parametrize("long_read_sees", (True, False))
def test_stop_rule_adversary(ctx, long_read_sees):
    """200 short reads, and one read invoked before everything and completed
    last: its column is the top one, its inv_pos the least."""
    R = 201
    reads = np.zeros(R, dtype=abi.SF_READ_DTYPE)
    reads["ok_pos"][:200] = 12 + 2 * np.arange(200)
    reads["inv_pos"][:200] = reads["ok_pos"][:200] - 1
    reads["ok_pos"][200], reads["inv_pos"][200] = 1000, 0
    reads["inv_time"], reads["ok_time"] = reads["inv_pos"] * C.MS, reads["ok_pos"] * C.MS
    adds = np.zeros(3, dtype=abi.SF_ADD_DTYPE)
    adds["value"], adds["inv_pos"], adds["ok_pos"] = [7, 8, 9], [1, 2, 3], [4, -1, 6]
    adds["ok_time"] = adds["ok_pos"].clip(0) * C.MS
    # 7: the short reads and the long one disagree about it; 8: only the long
    # read lists it, if any; 9: seen by short reads 0 .. 100, then missed
    if long_read_sees:
        per_read = [[9] * (c <= 100) for c in range(200)] + [[7, 8]]
    else:
        per_read = [[7] + [9] * (c <= 100) for c in range(200)] + [[9]]
    got, _ = _agree(ctx, adds, reads, C.payload_from(reads, per_read), what=long_read_sees)
    if long_read_sees:   # 7: present only at the long read (inv 0), absent up to inv 409
        assert (got["last_present"][0], got["last_absent"][0], got["outcome"][0]) == (0, 409, abi.LC_SF_LOST)
        assert (got["last_present"][1], got["last_absent"][1]) == (0, 409)
    else:                # 7: present up to inv 409, absent only at the long read: stable
        assert (got["last_present"][0], got["last_absent"][0], got["outcome"][0]) == (409, 0, abi.LC_SF_STABLE)
        assert (got["last_present"][1], got["last_absent"][1]) == (-1, 409)


def test_invoke_order_reversed_across_a_word_edge(ctx):
    """Columns 24 .. 40 complete in order and were invoked in the opposite order."""
    R = 70
    reads = np.zeros(R, dtype=abi.SF_READ_DTYPE)
    reads["ok_pos"] = 200 + 2 * np.arange(R)
    reads["inv_pos"] = reads["ok_pos"] - 1
    reads["inv_pos"][24:41] = 150 - np.arange(17)
    reads["inv_time"], reads["ok_time"] = reads["inv_pos"] * C.MS, reads["ok_pos"] * C.MS
    adds = np.zeros(4, dtype=abi.SF_ADD_DTYPE)
    adds["value"], adds["inv_pos"], adds["ok_pos"] = [1, 2, 3, 4], [0, 1, 2, 3], [10, 11, -1, -1]
    adds["ok_time"] = adds["ok_pos"].clip(0) * C.MS
    # 1: seen only by the reversed reads; 2: missed only by them; 3: seen by
    # columns 31 and 32 alone; 4: missed by columns 31 and 32 alone
    per_read = [[1] * (24 <= c <= 40) + [2] * (not 24 <= c <= 40) + [3] * (c in (31, 32)) +
                [4] * (c not in (31, 32)) for c in range(R)]
    got, _ = _agree(ctx, adds, reads, C.payload_from(reads, per_read))
    assert got["last_present"].tolist() == [150, 200 + 2 * 69 - 1, 143, 200 + 2 * 69 - 1]
    assert got["last_absent"].tolist() == [200 + 2 * 69 - 1, 150, 200 + 2 * 69 - 1, 143]


def test_table_collisions_and_extreme_values(ctx):
    E, cap = 40, 128
    same_slot = [v for v in range(1, 5000) if _slot(v, cap) == 5][:12]
    wrap = [v for v in range(1, 5000) if _slot(v, cap) == cap - 1][:4]   # the probe wraps round
    assert len(same_slot) == 12 and len(wrap) == 4
    low_bits = [5 + cap * k for k in range(1, 9)]
    extreme = [2 ** 63 - 1, -2 ** 63 + 1, -1, -5, 0, -cap + 5]
    pool = dict.fromkeys(same_slot + wrap + low_bits + extreme + list(range(300000, 300060)))
    values = np.array(list(pool)[:E], dtype=np.int64)
    adds, reads, vals = C.random_case(11, E, 50, element_values=values)
    # phantoms that land in the colliding chain, and the reserved value
    extra = np.array([v for v in range(200000, 205000) if _slot(v, cap) == 5][:6] + [-2 ** 63], dtype=np.int64)
    reads["off"][-1], reads["len"][-1] = len(vals), len(extra)   # the last read lists only these
    got, gs = _agree(ctx, adds, reads, np.concatenate([vals, extra]))
    assert gs["n_phantom"] >= len(extra)


def test_only_phantoms(ctx):
    adds, reads, _ = C.random_case(5, 20, 40, extras=False)
    per_read = [[10 ** 6 + c, 10 ** 6 + c] for c in range(40)]   # nobody added these (twice: no duplicate either)
    got, gs = _agree(ctx, adds, reads, C.payload_from(reads, per_read))
    assert gs["n_phantom"] == 80 and gs["n_stable"] == 0 and gs["n_duplicated"] == 0
    # elements listed only by reads that completed before their add
    adds, reads, values = C.ladder(70, 65, 3, "all")
    reads["len"][65:] = 0
    got, gs = _agree(ctx, adds, reads, values)
    assert gs["n_phantom"] == 3 * 65 and (got["last_present"] == -1).all()


def test_duplicates(ctx):
    adds, reads, values = C.ladder(40, 0, 3, "all")
    per_read = [[100, 101, 102] for _ in range(40)]
    per_read[3] = [100, 100, 101, 102]
    per_read[33] = [100, 101, 100, 102, 100, 102]
    per_read[39] = [102] * 5
    got, gs = _agree(ctx, adds, reads, C.payload_from(reads, per_read))
    assert got["dup_max"].tolist() == [3, 0, 5] and gs["n_duplicated"] == 2 and gs["valid"] == 0
    assert got["flags"].tolist() == [abi.LC_SF_DUPLICATED, 0, abi.LC_SF_DUPLICATED]
    # overlapping payload ranges are not duplicates
    reads["off"], reads["len"] = 0, 3
    got, gs = _agree(ctx, adds, reads, np.array([100, 101, 102], dtype=np.int64))
    assert gs["n_duplicated"] == 0 and gs["n_stable"] == 3


def test_random_histories(ctx):
    rng = np.random.default_rng(99)
    seen = dict.fromkeys(COUNTS[3:], 0)
    for i in range(300):
        E, R = int(rng.integers(0, 301)), int(rng.integers(0, 201))
        _, gs = _agree(ctx, *C.random_case(5000 + i, E, R), linearizable=bool(i % 3), what=i)
        for k in seen:
            seen[k] += gs[k]
    assert all(v >= 100 for v in seen.values()), seen


def test_large(ctx):
    _, gs = _agree(ctx, *C.random_case(77, 5000, 1000), tiles=1)
    assert gs["n_stable"] > 500 and gs["n_lost"] > 500 and gs["n_phantom"] > 1000


def test_tiles(ctx, monkeypatch):
    E, R = 257, 65
    case = C.random_case(123, E, R)
    row = 4 * ((R + 31) // 32)
    base, bs = _agree(ctx, *case, tiles=1)
    for tile_bytes, tiles in ((E * row, 1), (129 * row, 2), (37 * row, 7), (row, E), (1, E)):
        monkeypatch.setenv("LC_SF_TILE_BYTES", str(tile_bytes))
        assert abi.set_full_limits()["tile_bytes"] == tile_bytes
        got, gs = _agree(ctx, *case, tiles=tiles, what=tile_bytes)
        assert (got == base).all() and [gs[k] for k in COUNTS] == [bs[k] for k in COUNTS]
    monkeypatch.delenv("LC_SF_TILE_BYTES")
    _agree(ctx, *case, tiles=1)


def test_workspace_reuse(ctx):
    """Two calls of different sizes on one context, larger then smaller and
    back: nothing of an earlier call survives."""
    with abi.Context(device_mask=1) as c:
        for E, R in ((300, 200), (7, 3), (64, 64), (1000, 150), (2, 90)):
            _agree(c, *C.random_case(E + R, E, R), what=(E, R))
            _agree(c, *C.ladder(R, R // 2, 3, "all"), what=("ladder", R))
    # the mix of sizes flips while the total stays about the same: on a fresh
    # context the per-element arrays shrink and the per-read arrays grow, so
    # every array moves inside a workspace that does not grow, and back
    with abi.Context(device_mask=1) as c:
        for E, R in ((600, 8), (8, 600), (600, 8)):
            _agree(c, *C.random_case(E + R, E, R), what=("flip", E, R))


@pytest.mark.parametrize("name", sorted(EINVAL_CASES))
def test_einval_then_a_good_call(ctx, name):
    adds, reads, values = C.arrays(*EINVAL_CASES[name])
    with pytest.raises(abi.LcError) as e:
        ctx.set_full(adds, reads, values)
    assert e.value.code == -errno.EINVAL and "lc_set_full" in str(e.value)
    _agree(ctx, *GOOD, what="after " + name)


def test_two_adds_of_one_value_among_many(ctx):
    adds, reads, values = C.random_case(8, 500, 30)
    adds["value"][417] = adds["value"][3]
    with pytest.raises(abi.LcError) as e:
        ctx.set_full(adds, reads, values)
    assert e.value.code == -errno.EINVAL and "two adds of one value" in str(e.value)
    with pytest.raises(abi.LcError):
        abi.set_full_host(adds, reads, values)
    # found only after the device has worked: still nothing is written to out
    out = np.full(len(adds), -7, dtype=abi.SF_ELEMENT_DTYPE)
    rc = abi.lib().lc_set_full(ctx._h, abi._ptr(adds), len(adds), abi._ptr(reads), len(reads),
                               abi._ptr(values), len(values), 1, abi._ptr(out), None)
    assert rc == -errno.EINVAL and (out["outcome"] == -7).all() and (out["lost_latency_ms"] == -7).all()
    _agree(ctx, *C.random_case(8, 500, 30))


def test_empty_sides(ctx):
    for adds, reads, values in (([], GOOD[1], GOOD[2]), (GOOD[0], [], []), ([], [], [])):
        _, gs = _agree(ctx, adds, reads, values)
        assert gs["valid"] == -1


def test_checker_on_a_generated_history(ctx):
    h = REF.random_history(4040, max_elements=300, max_reads=200, n_procs=40, full=True)
    assert len({op["process"] for op in h if isinstance(op["process"], int)}) == 40
    dev = SF.SetFullChecker()
    try:
        got = dev.check({}, h, {})
    finally:
        dev.close()
    assert got == SF.SetFullChecker(device=False).check({}, h, {})
    assert got == REF.check(h)[1]
    assert got["attempt-count"] == 300 and got["stable-count"] > 50
