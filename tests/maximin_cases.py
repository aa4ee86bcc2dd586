"""What the maximin tests share (tests/test_rows_maximin_host.py on the CPU, tests/test_gpu_rows_maximin.py on
the device): the rounds of csa_rows_maximin_async's contract as a plain Python loop over dicts and member lists
(the yardstick of the numpy mirror stats.rows_maximin_host), the table generators, and the maximin LP itself
through scipy's HiGHS (tests only; the package never imports scipy).

Nothing here calls the device."""
import functools

import numpy as np

import price_cases as P
from conftest import pkg

NO_ROW = P.NO_ROW
PRICE_NONE = P.PRICE_NONE

# (D, n, k, shrink, rounds): the skewed tables, whose optimum is not the trivial k / covered
SKEWED = [(300, 20, 5, 0.8, 600), (1000, 70, 9, 0.8, 2000), (3000, 150, 20, 0.9, 5000)]


def pack(member_lists, n):
    """uint64[D, W] from lists of agent indices."""
    W = (n + 63) // 64
    rows = np.zeros((len(member_lists), W), np.uint64)
    for d, row in enumerate(member_lists):
        for p in row:
            rows[d, int(p) >> 6] |= np.uint64(1) << np.uint64(int(p) & 63)
    return rows


@functools.lru_cache(maxsize=None)
def skewed_rows(D, n, k, seed=0):
    """The distinct rows of D draws of k agents without replacement under cubed-uniform agent probabilities: some
    agents are in few panels, so the maximin optimum lies below k / covered."""
    rng = np.random.default_rng([D, n, k, seed, 7])
    p = rng.uniform(0.02, 1, n) ** 3
    p = p / p.sum()
    rows = np.unique(pack([rng.choice(n, k, replace=False, p=p) for _ in range(D)], n), axis=0)
    rows.setflags(write=False)
    return rows


def partition_rows(n, k):
    """n / k disjoint panels: row j holds agents [j k, (j + 1) k)."""
    assert n % k == 0
    return pack([range(j * k, (j + 1) * k) for j in range(n // k)], n)


def covered(rows, n):
    return sorted({i for row in P.members(rows, n) for i in row})


def lane_sum(w, n, W):
    partial = [0.0] * 64
    for j in range(W):
        for lane in range(64):
            partial[lane] = partial[lane] + (w[64 * j + lane] if 64 * j + lane < n else 0.0)
    total = 0.0
    for lane in range(64):
        total = total + partial[lane]
    return total


def _scores(mem, w):
    out = []
    for row in mem:
        s = 0.0
        for i in row:
            s = s + w[i]
        out.append(s)
    return out


def _best(scores):
    at, value = None, None
    for d, s in enumerate(scores):
        if at is None or s > value:
            at, value = d, s
    return at, value


def maximin_loop(mem, n, W, rounds, shrink=0.8, resync=16, state=None, descending=False):
    """The contract over dicts and lists: ``(picks, state)`` with state = dict(weights, scores, cover, row_count,
    upper, rounds, best_row, ratio); ``state`` given: continued (a copy).  ``descending``: the intersection sums
    of the update pass run in descending agent order, for the order-sensitivity condition."""
    D = len(mem)
    if state is None:
        held = {i for row in mem for i in row}
        w = {i: (1.0 if i in held else 0.0) for i in range(n)}
        cover, row_count, done = {i: 0 for i in range(n)}, [0] * D, 0
        scores = _scores(mem, w)
        best_row, upper, ratio = PRICE_NONE, float("inf"), float("inf")
        if D:
            best_row, value = _best(scores)
            upper = ratio = value / lane_sum(w, n, W)
    else:
        w = {i: float(x) for i, x in enumerate(state["weights"])}
        cover = {i: int(x) for i, x in enumerate(state["cover"])}
        row_count, scores = [int(x) for x in state["row_count"]], [float(x) for x in state["scores"]]
        upper, done, best_row, ratio = state["upper"], state["rounds"], state["best_row"], state["ratio"]
    picks = []
    for r in range(rounds):
        if not D:
            picks.append(NO_ROW)
            continue
        at, _ = _best(scores)
        picks.append(at)
        row_count[at] += 1
        done += 1
        delta = {}
        for i in mem[at]:
            v = w[i] * shrink
            delta[i] = w[i] - v
            w[i] = v
            cover[i] += 1
        if (r + 1) % resync != 0 and r != rounds - 1:
            for d, row in enumerate(mem):
                t = 0.0
                for i in (reversed(row) if descending else row):
                    if i in delta:
                        t = t + delta[i]
                scores[d] = scores[d] - t
            continue
        f = float(n) / lane_sum(w, n, W)
        for i in range(n):
            w[i] = w[i] * f
        scores = _scores(mem, w)
        best_row, value = _best(scores)
        ratio = value / lane_sum(w, n, W)
        if ratio < upper:
            upper = ratio
    return picks, {"weights": np.array([w[i] for i in range(n)], np.float64), "scores": np.array(scores, np.float64),
                   "cover": np.array([cover[i] for i in range(n)], np.int64), "row_count": np.array(row_count, np.int64),
                   "upper": upper, "rounds": done, "best_row": best_row, "ratio": ratio}


def forged_order_state(rows, n, p0, shrink=0.8, salt=0):
    """A state that makes the order of the update pass's sums decide a pick (price_cases' order-sensitive idea
    carried to the intersections): positive weights spread over 2^-20 .. 2^20, and scores[d] = the ascending sum of
    the deltas a pick of row p0 causes over row d's intersection with it.  Row p0 holds the greatest score, so it
    is picked first; the update pass then leaves exactly +0.0 everywhere when it sums in ascending order -- the
    second pick is row 0 -- and a last-bit residue where another order rounds differently."""
    rng = np.random.default_rng([len(rows), n, p0, salt, 11])
    w = rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-20, 21, n).astype(np.float64))
    mem = P.members(rows, n)
    delta = {}
    for i in mem[p0]:
        wi = float(w[i])
        delta[i] = wi - wi * shrink
    scores = []
    for row in mem:
        t = 0.0
        for i in row:
            if i in delta:
                t = t + delta[i]
        scores.append(t)
    return {"weights": w, "scores": np.array(scores, np.float64), "cover": np.zeros(n, np.int64),
            "row_count": np.zeros(len(rows), np.int64), "upper": float("inf"), "rounds": 0, "best_row": p0,
            "ratio": float("inf")}


def same_state(got, want):
    """A stats.MaximinState against the loop's dict, bit for bit; the reason for a difference, or None."""
    for name in ("weights", "scores"):
        if not np.array_equal(P.bits(getattr(got, name)), P.bits(want[name])):
            return name
    for name in ("cover", "row_count"):
        if not np.array_equal(np.asarray(getattr(got, name), np.int64), want[name]):
            return name
    for name in ("upper", "ratio"):
        if P.bits1(getattr(got, name)) != P.bits1(want[name]):
            return name
    if (got.rounds, got.best_row) != (want["rounds"], want["best_row"]):
        return "rounds / best_row"
    return None


def state_dict(state):
    """A stats.MaximinState as the loop's dict."""
    return {name: getattr(state, name) for name in state._fields}


@functools.lru_cache(maxsize=None)
def lp_optimum(D, n, k, seed=0):
    """z* of the maximin LP over skewed_rows(D, n, k, seed): maximise z s.t. the sum of x_P over the rows holding
    i >= z for every covered agent i, the x_P sum to 1, x >= 0.  HiGHS through scipy."""
    import pytest
    opt = pytest.importorskip("scipy.optimize")
    rows = skewed_rows(D, n, k, seed)
    return lp_over(rows, n, opt)


def lp_over(rows, n, opt=None):
    if opt is None:
        import pytest
        opt = pytest.importorskip("scipy.optimize")
    member = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(np.float64)
    held = np.flatnonzero(member.any(axis=0))
    d = len(rows)
    a_ub = np.hstack([-member[:, held].T, np.ones((len(held), 1))])        # z - sum over P holding i of x_P <= 0
    a_eq = np.hstack([np.ones((1, d)), np.zeros((1, 1))])
    c = np.zeros(d + 1)
    c[d] = -1.0
    res = opt.linprog(c, A_ub=a_ub, b_ub=np.zeros(len(held)), A_eq=a_eq, b_eq=[1.0],
                      bounds=[(0, None)] * d + [(None, None)], method="highs")
    assert res.status == 0, res.message
    return float(-res.fun)


@functools.lru_cache(maxsize=None)
def mirror(D, n, k, shrink, rounds, resync=16, seed=0):
    """stats.rows_maximin_host over a skewed table, once."""
    return pkg("stats").rows_maximin_host(skewed_rows(D, n, k, seed), n, rounds, shrink, resync)


def lower_bound(state, rounds):
    """min over covered agents of cover / rounds as a Fraction (covered = weight not zero)."""
    from fractions import Fraction
    return min(Fraction(int(c), rounds) for c, w in zip(state.cover, state.weights) if w != 0.0)
