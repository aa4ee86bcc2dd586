"""What the table-join tests share (tests/test_rows_join_host.py on the CPU, tests/test_gpu_rows_join.py on the
device): the join and the lookup by np.unique and Counter over ``bytes(row)`` alone, query batches for the
lookup, and a portfolio beside a run with its overlap figures written out as a loop.

The expected values never come from the code under test."""
from collections import Counter

import numpy as np

SELECTS = [0, 1, 2, 3, 4, 7]
MISSING = 0xFFFFFFFF
COUPLES = "couples_panel_from_twenty_people_no_constraints_2"


def _counts(t):
    rows, mult = t
    mult = [1] * len(rows) if mult is None else [int(m) for m in mult]
    c = Counter()
    for r, m in zip(rows, mult):
        c[bytes(r)] += m
    assert len(c) == len(rows)          # a table's rows are distinct
    return c


def np_join(a, b, select, scales=(1, 1)):
    """(rows, mult_a, mult_b, length, record) of tables ``a`` and ``b``, each ``(rows uint64[n, W], mult or
    None)``: the rows of the sorted union whose class (1 only in a, 2 only in b, 4 in both) is in ``select``, their
    multiplicities on either side, their number, and the 11 integers over the whole union."""
    ca, cb = _counts(a), _counts(b)
    sa, sb = (int(s) for s in scales)
    W = a[0].shape[1]
    both = np.concatenate([np.ascontiguousarray(a[0], np.uint64), np.ascontiguousarray(b[0], np.uint64)])
    union = np.unique(both, axis=0) if len(both) else both
    keys = [bytes(r) for r in union]
    cls = [4 if k in ca and k in cb else 1 if k in ca else 2 for k in keys]
    shared = [k for k, c in zip(keys, cls) if c == 4]
    cross = sum(ca[k] * cb[k] for k in shared)
    overlap = sum(min(ca[k] * sb, cb[k] * sa) for k in shared)
    record = [len(keys), len(shared), cls.count(1), cls.count(2), sum(ca.values()), sum(cb.values()),
              sum(ca[k] for k in shared), sum(cb[k] for k in shared), cross % 2 ** 64, overlap % 2 ** 64,
              int(cross >= 2 ** 64 or overlap >= 2 ** 64)]
    keep = [i for i, c in enumerate(cls) if c & select]
    return (union[keep].reshape(-1, W), np.array([ca.get(keys[i], 0) for i in keep], np.int64),
            np.array([cb.get(keys[i], 0) for i in keep], np.int64), len(keep), record)


def np_find(table_rows, queries):
    at = {bytes(r): i for i, r in enumerate(table_rows)}
    return np.array([at.get(bytes(q), MISSING) for q in queries], np.int64)


def find_table(W, n=2 * 1024 + 77):
    """A sorted distinct table of ``n`` rows, about half of them with bit 63 of word 0 set."""
    rng = np.random.default_rng([n, W, 11])
    rows = np.unique(rng.integers(0, 1 << 64, size=(n + 64, W), dtype=np.uint64), axis=0)[:n]
    assert len(rows) == n and (rows[-1, 0] >> np.uint64(63)) == 1 and (rows[0, 0] >> np.uint64(63)) == 0
    return rows


def query_batches(table):
    """name -> uint64[q, W] queries over a table of find_table's kind."""
    n, W = table.shape
    rng = np.random.default_rng([n, W, 12])
    present = table[rng.integers(0, n, size=300)]
    absent = rng.integers(0, 1 << 64, size=(300, W), dtype=np.uint64)
    near = table[rng.integers(0, n, size=100)].copy()
    near[:, W - 1] ^= np.uint64(1)                      # equal to a table row but for the last word's low bit
    below, above = table[:1].copy(), table[-1:].copy()
    below[0, W - 1] -= np.uint64(1)
    above[0, W - 1] += np.uint64(1)
    assert below[0, W - 1] != np.uint64(0xFFFFFFFFFFFFFFFF) and above[0, W - 1] != 0      # no wrap-around
    top = table[table[:, 0] >> np.uint64(63) == 1]
    top_absent = top[:50].copy()
    top_absent[:, 0] ^= np.uint64(1 << 62)
    out = {
        "present": present,
        "absent": np.concatenate([absent, near]),
        "duplicates": np.repeat(np.concatenate([present[:5], absent[:5]]), 7, axis=0),
        "ends": np.concatenate([below, above, table[:1], table[-1:], np.zeros((1, W), np.uint64),
                                np.full((1, W), 0xFFFFFFFFFFFFFFFF, np.uint64)]),
        "top_bit": np.concatenate([top[::37], top_absent]),
        "none": table[:0],
    }
    want = {k: np_find(table, q) for k, q in out.items()}
    assert (want["present"] != MISSING).all() and (want["absent"] == MISSING).all()
    assert want["ends"].tolist() == [MISSING, MISSING, 0, n - 1, MISSING, MISSING]
    assert (want["top_bit"] != MISSING).any() and (want["top_bit"] == MISSING).any()
    return out, want


def tuples(rows, ids):
    """Packed rows -> the set of agent-id tuples, members in ascending position."""
    n = len(ids)
    return {tuple(ids[q] for q in np.flatnonzero(np.unpackbits(r.view(np.uint8), bitorder="little")[:n]))
            for r in np.ascontiguousarray(rows, np.uint64)}


def counter_comparison(pa, pb):
    """The 11 record integers of two runs' panels (uint64[S, W] each) by Counter arithmetic in Python integers."""
    ca, cb = Counter(bytes(r) for r in pa), Counter(bytes(r) for r in pb)
    sa, sb = len(pa), len(pb)
    shared = [k for k in ca if k in cb]
    cross = sum(ca[k] * cb[k] for k in shared)
    overlap = sum(min(ca[k] * sb, cb[k] * sa) for k in shared)
    assert cross < 2 ** 64 and overlap < 2 ** 64
    return [len(set(ca) | set(cb)), len(shared), len(ca) - len(shared), len(cb) - len(shared), sa, sb,
            sum(ca[k] for k in shared), sum(cb[k] for k in shared), cross, overlap, 0]


def check_comparison(c, pa, pb):
    """Every integer and every figure of PanelComparison ``c`` against the Counter arithmetic."""
    want = counter_comparison(pa, pb)
    sa, sb = len(pa), len(pb)
    assert c.record == want and (c.S_a, c.S_b) == (sa, sb)
    assert (c.union, c.shared, c.only_a, c.only_b) == tuple(want[:4])
    ok = sa > 0 and sb > 0
    assert c.jaccard() == (want[1] / want[0] if ok and want[0] else 0.0)
    assert c.mass_a_on_b() == (want[6] / sa if ok else 0.0) and c.mass_b_on_a() == (want[7] / sb if ok else 0.0)
    assert c.overlap() == (want[9] / (sa * sb) if ok else 0.0)
    assert c.total_variation() == (1 - want[9] / (sa * sb) if ok else 0.0)
    assert c.cross_collision() == (want[8] / (sa * sb) if ok else 0.0)
    return want


def portfolio_case(panels, n, k):
    """A portfolio beside the run ``panels`` (uint64[S, W] over n agents, panels of k): 40 drawn panels, 10
    k-subsets never drawn, 3 entries repeated, shuffled, with random normalised weights.  Returns
    (rows uint64[53, W], weights float64[53])."""
    rng = np.random.default_rng(2024)
    drawn = np.unique(panels, axis=0)
    seen = {bytes(r) for r in drawn}
    picked = drawn[rng.permutation(len(drawn))[:40]]
    fresh = []
    while len(fresh) < 10:
        row = np.zeros(panels.shape[1], np.uint64)
        for q in rng.permutation(n)[:k]:
            row[q >> 6] |= np.uint64(1) << np.uint64(q & 63)
        if bytes(row) not in seen:
            seen.add(bytes(row))
            fresh.append(row)
    rows = np.concatenate([picked, np.array(fresh, np.uint64), picked[[3, 17]], np.array(fresh[4:5], np.uint64)])
    assert len(picked) == 40 and len(rows) == 53
    rows = rows[rng.permutation(len(rows))]
    w = rng.random(len(rows))
    return rows, w / w.sum()


def overlap_loop(panels, rows, weights):
    """The PortfolioOverlap figures as a plain loop: float64 adds from 0., left to right, in portfolio order;
    the distinct panels in the order of their first entry."""
    S = len(panels)
    drawn = Counter(bytes(r) for r in panels)
    counts = [drawn.get(bytes(r), 0) for r in rows]
    mass_seen = 0.
    for m, w in zip(counts, weights.tolist()):
        if m > 0:
            mass_seen += w
    distinct = {}
    for r, m, w in zip(rows, counts, weights.tolist()):
        if bytes(r) in distinct:
            distinct[bytes(r)][1] += w
        else:
            distinct[bytes(r)] = [m, w]
    overlap = 0.
    for m, w in distinct.values():
        overlap += min(m / S, w)
    return {"counts": counts, "panels": len(distinct), "panels_seen": sum(1 for m, _ in distinct.values() if m > 0),
            "legacy_mass": sum(m for m, _ in distinct.values()) / S, "portfolio_mass_seen": mass_seen,
            "overlap": overlap}


def check_overlap(po, want):
    assert po.counts.tolist() == want["counts"]
    assert (po.panels, po.panels_seen) == (want["panels"], want["panels_seen"])
    for name in ("legacy_mass", "portfolio_mass_seen", "overlap"):
        assert getattr(po, name) == want[name], name            # bit-equal floats
