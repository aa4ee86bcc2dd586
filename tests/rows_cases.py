"""What the sorted distinct-row tests share (tests/test_rows_host.py on the CPU, tests/test_gpu_rows_sort.py
on the device): builders of uint64[n, W] row batches, one per content family, pairs of sorted tables for the
merge, and numpy's own answer.  Every builder is deterministic in (n, W).

The expected values never come from the code under test: ``np_table`` is
np.unique(rows, axis=0, return_index=True, return_counts=True), whose row order (word 0 most significant,
unsigned 64-bit compare) is the order the tables promise."""
import numpy as np

WIDTHS = [1, 2, 27, 128]
MERGE_TILE = 1024          # rs_merge_kernel's output tile (== csa_rows_sort_tile(); asserted by the GPU test)


def _rng(n, W, salt):
    return np.random.default_rng([n, W, salt])


def _fresh(rng, n, W):
    return rng.integers(0, 1 << 64, size=(n, W), dtype=np.uint64)


def dup_pool(n, W):
    """About 3/4 duplicates: rows drawn from a pool of ~n/4 rows, permuted so copies land in different tiles."""
    rng = _rng(n, W, 1)
    pool = _fresh(rng, max(n // 4, 1), W)
    rows = pool[np.arange(n) % len(pool)]
    return rows[rng.permutation(n)]


def all_equal(n, W):
    return np.repeat(_fresh(_rng(n, W, 2), 1, W), n, axis=0)


def shared_prefix(n, W):
    """All rows distinct, sharing words 0 .. W-2: every compare runs the full length (W = 1: distinct words)."""
    rng = _rng(n, W, 3)
    rows = np.repeat(_fresh(rng, 1, W), n, axis=0)
    rows[:, W - 1] = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15 if W > 1 else 7919)
    return rows


def top_bit(n, W):
    """Half the rows with bit 63 of word 0 set: a signed compare would order them first."""
    rng = _rng(n, W, 4)
    rows = _fresh(rng, n, W) >> np.uint64(1)
    rows[::2, 0] |= np.uint64(1 << 63)
    return rows


def ascending(n, W):
    rows = _fresh(_rng(n, W, 5), n, W)
    return np.unique(rows, axis=0) if n else rows


def descending(n, W):
    return ascending(n, W)[::-1].copy()


def low_bit(n, W):
    """Rows differing only in bit 0 of word 0 (two distinct rows, interleaved irregularly)."""
    rng = _rng(n, W, 6)
    rows = np.repeat(_fresh(rng, 1, W), n, axis=0)
    rows[:, 0] = (rows[:, 0] & ~np.uint64(1)) | rng.integers(0, 2, size=n, dtype=np.uint64)
    return rows


FAMILIES = {"dup_pool": dup_pool, "all_equal": all_equal, "shared_prefix": shared_prefix, "top_bit": top_bit,
            "ascending": ascending, "descending": descending, "low_bit": low_bit}


def sizes(T):
    """A partial tile, a run with no partner in a merge pass, at least three merge levels."""
    return [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5, 8 * T + 3]


def np_table(rows, index_base=0):
    """(rows, first, mult) by numpy alone."""
    rows = np.ascontiguousarray(rows, np.uint64)
    if len(rows) == 0:
        return rows.copy(), np.zeros(0, np.int64), np.zeros(0, np.int64)
    u, f, m = np.unique(rows, axis=0, return_index=True, return_counts=True)
    return u, f.astype(np.int64) + index_base, m.astype(np.int64)


def _table(rng, rows, lo):
    """A sorted distinct table over ``rows`` with arbitrary firsts (from ``lo`` up) and mults."""
    u = np.unique(rows, axis=0) if len(rows) else rows
    return u, lo + rng.permutation(len(u)).astype(np.int64), rng.integers(1, 1000, size=len(u)).astype(np.int64)


def merge_pairs(W, M=MERGE_TILE):
    """name -> (A, B), each (rows, first, mult) sorted and distinct; lengths straddle the merge tile M."""
    rng = _rng(M, W, 7)
    base = np.unique(_fresh(rng, 2 * M + 77, W), axis=0)
    empty = base[:0]
    lowhalf, highhalf = base[:M + 1], base[M + 1:]
    out = {
        "a_empty": (_table(rng, empty, 0), _table(rng, base[:M + 3], 10)),
        "b_empty": (_table(rng, base[:M - 1], 0), _table(rng, empty, 10)),
        "both_empty": (_table(rng, empty, 0), _table(rng, empty, 0)),
        "equal": (_table(rng, base[:M + 5], 0), _table(rng, base[:M + 5], 5000)),
        "interleaved": (_table(rng, base[0::2], 0), _table(rng, base[1::2], 7)),
        "a_below_b": (_table(rng, lowhalf, 100), _table(rng, highhalf, 0)),
        "overlap": (_table(rng, base[:M + 9], 3), _table(rng, base[M // 2:2 * M + 1], 0)),
        "tiny": (_table(rng, base[5:6], 9), _table(rng, base[5:7], 2)),
    }
    return out


MERGE_NAMES = ["a_empty", "b_empty", "both_empty", "equal", "interleaved", "a_below_b", "overlap", "tiny"]


def np_merge(a, b):
    """The union by numpy alone: sort-unique of the concatenation, first the minimum, mult the sum."""
    rows = np.concatenate([a[0], b[0]])
    if len(rows) == 0:
        return rows, np.zeros(0, np.int64), np.zeros(0, np.int64)
    u, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    f, m = np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]])
    first = np.array([f[inv == e].min() for e in range(len(u))], np.int64)
    mult = np.array([m[inv == e].sum() for e in range(len(u))], np.int64)
    return u, first, mult
