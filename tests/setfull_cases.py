"""lc_set_full inputs as flat arrays, made with numpy for the GPU tests: any
number of elements and reads, every element with a story of its own (always
seen, never seen, seen from some read on, seen up to some read, seen at
random), plus phantoms and duplicates."""
import numpy as np

from jepsen.etcd_amd import abi

MS = 1_000_000


def arrays(adds, reads, values):
    return (np.ascontiguousarray(adds, dtype=abi.SF_ADD_DTYPE),
            np.ascontiguousarray(reads, dtype=abi.SF_READ_DTYPE),
            np.ascontiguousarray(values, dtype=np.int64))


def payload_from(reads, per_read):
    """Fill off / len of `reads` from a list of per-read value lists."""
    lens = np.array([len(p) for p in per_read], dtype=np.int64)
    reads["len"] = lens
    reads["off"] = np.cumsum(lens) - lens
    flat = [x for p in per_read for x in p]
    return np.array(flat, dtype=np.int64)


def random_case(seed, n_elements, n_reads, extras=True, element_values=None):
    """(adds, reads, values).  Positions are distinct over the whole history;
    the concerning columns of an element start anywhere in its row."""
    rng = np.random.default_rng(seed)
    E, R = n_elements, n_reads
    pos = rng.permutation(2 * (E + R) + 8)[:2 * (E + R)].astype(np.int64).reshape(-1, 2)
    pos.sort(axis=1)
    a_pos, r_pos = pos[:E], pos[E:]
    a_pos = a_pos[np.argsort(a_pos[:, 0])]
    r_pos = r_pos[np.argsort(r_pos[:, 1])]
    adds = np.zeros(E, dtype=abi.SF_ADD_DTYPE)
    if element_values is None:
        element_values = rng.permutation(4 * E + 4)[:E].astype(np.int64) - E
    adds["value"] = element_values
    adds["inv_pos"] = a_pos[:, 0]
    has_ok = rng.random(E) < 0.7
    adds["ok_pos"] = np.where(has_ok, a_pos[:, 1], -1)
    jitter = lambda p: p * 400_000 + rng.integers(0, 400_000, len(p))  # noqa: E731
    adds["ok_time"] = np.where(has_ok, jitter(a_pos[:, 1]), 0)
    reads = np.zeros(R, dtype=abi.SF_READ_DTYPE)
    reads["inv_pos"], reads["ok_pos"] = r_pos[:, 0], r_pos[:, 1]
    reads["inv_time"], reads["ok_time"] = jitter(r_pos[:, 0]), jitter(r_pos[:, 1])
    # who lists what: a story per element
    story = rng.integers(0, 5, E)
    turn = rng.integers(0, max(R, 1) + 1, E)
    col = np.arange(R)[:, None]
    seen = np.select([story[None, :] == 0, story[None, :] == 1, story[None, :] == 2, story[None, :] == 3],
                     [np.ones((R, E), bool), np.zeros((R, E), bool), col >= turn[None, :], col < turn[None, :]],
                     rng.random((R, E)) < 0.5)
    if not extras:  # only what concerns: no phantoms
        seen &= reads["ok_pos"][:, None] > adds["inv_pos"][None, :]
    rr, ee = np.nonzero(seen)
    vals = adds["value"][ee]
    if extras and R:
        # any element again (a duplicate where the read lists it, a phantom where
        # it does not concern), and values nobody added
        n_x = int(rng.integers(0, 2 * R + 1))
        xr = rng.integers(0, R, n_x)
        xv = np.where(rng.random(n_x) < 0.6, adds["value"][rng.integers(0, E, n_x)] if E else 0,
                      rng.integers(10 * E + 10, 20 * E + 20, n_x))
        rr, vals = np.concatenate([rr, xr]), np.concatenate([vals, xv])
    order = np.argsort(rr, kind="stable")
    rr, vals = rr[order], vals[order]
    lens = np.bincount(rr, minlength=R).astype(np.int64)
    reads["len"] = lens
    reads["off"] = np.cumsum(lens) - lens
    return adds, reads, vals.astype(np.int64)


def ladder(n_reads, first_column, n_elements=1, seen="all"):
    """Reads with ok_pos 10, 12, ... and n_elements adds whose inv_pos lies just
    below read `first_column`'s ok_pos and above the one before: the concerning
    suffix starts exactly at that column.  seen: "all" / "none" / "odd"."""
    R = n_reads
    reads = np.zeros(R, dtype=abi.SF_READ_DTYPE)
    reads["ok_pos"] = 10 + 2 * np.arange(R) * max(n_elements, 1)
    reads["inv_pos"] = reads["ok_pos"] - 1
    reads["inv_time"], reads["ok_time"] = reads["inv_pos"] * MS, reads["ok_pos"] * MS
    adds = np.zeros(n_elements, dtype=abi.SF_ADD_DTYPE)
    lo = reads["ok_pos"][first_column - 1] if first_column > 0 else 0
    adds["inv_pos"] = lo + 1 + np.arange(n_elements) if first_column > 0 else np.arange(n_elements)
    adds["ok_pos"] = -1
    adds["value"] = 100 + np.arange(n_elements)
    per_read = []
    for c in range(R):
        if seen == "all" or (seen == "odd" and c % 2):
            per_read.append(adds["value"].tolist())  # below first_column these are phantoms
        else:
            per_read.append([])
    return adds, reads, payload_from(reads, per_read)
