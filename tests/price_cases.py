"""What the pricing tests share (tests/test_rows_price_host.py on the CPU, tests/test_gpu_rows_price.py on the
device): weight vectors, tables of random k-subsets, the C oracle's tables, plain Python loops over unpacked
member lists -- the yardsticks of the numpy mirrors -- and the mirrors' own results on the larger tables,
computed once and shared.

Nothing here calls the device.  The loops are transcriptions of the contract (the sum of a row's weights in
ascending agent index from +0.0; the multiplicative-weights round in the order of the reference's
xmin.py:251-266 with the lane-strided weight sum), written over dicts and lists, not numpy."""
import functools

import numpy as np

from conftest import inst_paths, pkg
from multiplicity_cases import oracle_panels

COUPLES = "couples_panel_from_twenty_people_no_constraints_2"
NO_ROW = 0xFFFFFFFF
PRICE_NONE = 0xFFFFFFFFFFFFFFFF
WEIGHTS = ["normal", "equal", "order", "zeros"]

# name -> (instance, k, S, seed, rounds): the multiplicative-weights tables
COVER_TABLES = {"example_small_20": ("example_small_20", 20, 3000, 0, 600),
                "couples": (COUPLES, 2, 500, 0, 60),
                "sf_e_110": ("sf_e_110", 110, 300, 0, 60)}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits1(x):
    """One float64's bits as an int."""
    return int(np.array([x], np.float64).view(np.uint64)[0])


def weights(name, n, salt=0):
    """float64[n].  normal: positive, spread over a decade.  equal: every score of a k-subset table ties.
    order: magnitudes over about 2^-40 .. 2^40 with mixed signs, so the order of a sum shows in its bits.
    zeros: +0.0 and -0.0 mixed with a few ordinary values."""
    rng = np.random.default_rng([n, salt, WEIGHTS.index(name)])
    if name == "normal":
        return rng.uniform(0.1, 1.0, n)
    if name == "equal":
        return np.full(n, 0.37)
    if name == "order":
        return rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-40, 41, n).astype(np.float64))
    w = np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0)
    w[rng.integers(0, n, max(n // 8, 1))] = 0.25
    return w


def subset_rows(D, W, n, k=None, salt=0, low=0):
    """uint64[D, W]: random k-subsets of the agents [low, n), padding bits zero."""
    k = max(1, min((n - low) // 3, 40)) if k is None else k
    rng = np.random.default_rng([D, W, n, k, salt])
    rows = np.zeros((D, W), np.uint64)
    for d in range(D):
        for p in rng.choice(n - low, k, replace=False) + low:
            rows[d, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    return rows


def members(rows, n):
    """Per row the ascending list of its agents."""
    rows = np.ascontiguousarray(rows, np.uint64)
    if not len(rows):
        return []
    m = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :n]
    return [np.flatnonzero(r).tolist() for r in m]


def score_loop(mem, w, descending=False):
    """The contract in plain Python: per row the float sum from +0.0 over its members in ascending index
    (``descending``: the other order, for the order-sensitivity condition)."""
    w = [float(x) for x in w]
    out = []
    for row in mem:
        s = 0.0
        for i in (reversed(row) if descending else row):
            s = s + w[i]
        out.append(s)
    return np.array(out, np.float64)


def best_loop(scores, index_base=0, stored=None):
    """(index, value): a scan in ascending row order replacing on ``>`` alone; ``stored`` = an (index, value)
    carried in (accumulate): replaced only by a strictly greater score, or when it is PRICE_NONE."""
    at, value = PRICE_NONE, -np.inf
    for d, s in enumerate(np.asarray(scores, np.float64).tolist()):
        if at == PRICE_NONE or s > value:
            at, value = d + index_base, s
    if stored is not None and (at == PRICE_NONE or not (stored[0] == PRICE_NONE or value > stored[1])):
        return stored
    return at, value


def assert_order_sensitive(rows, n, w):
    """A condition on the input: summing some row's members in descending order gives other bits."""
    mem = members(rows, n)
    up, down = score_loop(mem, w), score_loop(mem, w, descending=True)
    assert (bits(up) != bits(down)).any(), "the order-sensitive weights do not distinguish summation orders here"


def first_holder_loop(mem, n):
    out = [NO_ROW] * n
    for d, row in enumerate(mem):
        for i in row:
            if out[i] == NO_ROW:
                out[i] = d
    return np.array(out, np.int64)


def mw_cover_loop(mem, n, W, rounds, w=None, chosen=None):
    """The multiplicative-weights rounds over dicts and lists: (picks, weights, chosen set, pick scores,
    repeat rounds)."""
    w = {i: 1.0 for i in range(n)} if w is None else {i: float(x) for i, x in enumerate(w)}
    chosen = set() if chosen is None else set(chosen)
    picks, scores, repeats = [], [], 0
    for _ in range(rounds):
        if not mem:
            picks.append(NO_ROW)
            scores.append(-np.inf)
            continue
        best, value = None, None
        for d, row in enumerate(mem):
            s = 0.0
            for i in row:
                s = s + w[i]
            if best is None or s > value:
                best, value = d, s
        picks.append(best)
        scores.append(value)
        for i in mem[best]:
            w[i] *= 0.8
        partial = [0.0] * 64
        for j in range(W):
            for lane in range(64):
                partial[lane] = partial[lane] + (w[64 * j + lane] if 64 * j + lane < n else 0.0)
        total = 0.0
        for lane in range(64):
            total = total + partial[lane]
        for i in range(n):
            w[i] *= n / total
        if best in chosen:
            repeats += 1
            for i in range(n):
                w[i] = 0.9 * w[i] + 0.1
        else:
            chosen.add(best)
    return picks, np.array([w[i] for i in range(n)], np.float64), chosen, np.array(scores, np.float64), repeats


def committees_loop(mem, n, ids, picks):
    """The reference's return shape from picks over member lists: the picked panels, then per agent in order the
    lowest row holding it when nothing covers it yet (xmin.py:272-282's counterpart)."""
    committees, covered, lines = set(), set(), []
    for p in picks:
        if p != NO_ROW:
            committees.add(frozenset(ids[i] for i in mem[p]))
            covered |= {ids[i] for i in mem[p]}
    for i in range(n):
        if ids[i] in covered:
            continue
        holder = next((d for d, row in enumerate(mem) if i in row), None)
        if holder is None:
            lines.append("Agent %s not contained in any drawn panel." % (ids[i],))
            continue
        committees.add(frozenset(ids[q] for q in mem[holder]))
        covered |= {ids[q] for q in mem[holder]}
    if len(covered) == n:
        lines.append("All agents are contained in some drawn panel.")
    return committees, frozenset(covered), lines


@functools.lru_cache(maxsize=None)
def instance(name, k):
    inst = pkg().read_instance(*inst_paths(name), k)
    ids = list(pkg("analysis").encode_cached(inst.categories, inst.agents).agent_ids)
    return inst, ids


@functools.lru_cache(maxsize=None)
def oracle_table(name, k, seed, S):
    """(panels uint64[S, W], rows, first, mult): the C oracle's draws and their sorted distinct table."""
    panels = oracle_panels(name, k, seed, S)
    rows, first, mult = np.unique(panels, axis=0, return_index=True, return_counts=True)
    for a in (panels, rows, first, mult):
        a.setflags(write=False)
    return panels, rows, first.astype(np.int64), mult.astype(np.int64)


@functools.lru_cache(maxsize=None)
def cover(table):
    """The mirror's multiplicative-weights run over a COVER_TABLES entry, once: dict with the table's rows, n,
    the rounds, and rows_mw_cover_host's (picks, weights, chosen, scores) from unit weights."""
    name, k, S, seed, rounds = COVER_TABLES[table]
    _, ids = instance(name, k)
    rows = oracle_table(name, k, seed, S)[1]
    n = len(ids)
    picks, w, chosen, scores = pkg("stats").rows_mw_cover_host(rows, np.ones(n), np.zeros(len(rows), np.uint8), rounds)
    for a in (picks, w, chosen, scores):
        a.setflags(write=False)
    return {"rows": rows, "n": n, "rounds": rounds, "picks": picks, "weights": w, "chosen": chosen, "scores": scores,
            "repeats": rounds - len(set(picks.tolist()))}
