"""What the Nash-welfare tests share (tests/test_rows_nash_host.py on the CPU, tests/test_gpu_rows_nash.py on the
device): the contract of csa_rows_marginals_async and csa_rows_nash_async as a plain Python loop over member
lists and floats (the yardstick of the numpy mirrors stats.rows_marginals_host / stats.rows_nash_host), the
tables, and exact-rational recomputations of the marginals, the scores and the certificate from a given p.

Nothing here calls the device."""
import functools
import math
from fractions import Fraction

import numpy as np

import maximin_cases as M
import price_cases as P
from conftest import pkg

PRICE_NONE = P.PRICE_NONE
TILE = 1024

# name -> (D, n, k) of maximin_cases.skewed_rows: W = 1 (261 rows), W = 2 (n no multiple of 64), W = 3 (three tiles)
SHAPES = {"W1": (300, 20, 5), "W2": (1000, 70, 9), "W3": (3000, 150, 20)}


def table(name):
    """(rows, n) of a SHAPES entry."""
    D, n, k = SHAPES[name]
    return M.skewed_rows(D, n, k), n


def mults(D, salt=0):
    """int64[D] multiplicities 1 .. about 400, most of them small (a run's spectrum), and their sum."""
    rng = np.random.default_rng([D, salt, 13])
    m = np.maximum(1, (rng.uniform(0.0, 1.0, D) ** 6 * 400).astype(np.int64))
    m.setflags(write=False)
    return m, int(m.sum())


def spread_prob(D, salt=0):
    """float64[D]: positive weights spread over 2^-20 .. 2^20, so the order of a sum shows in its bits."""
    rng = np.random.default_rng([D, salt, 17])
    return rng.uniform(1.0, 2.0, D) * np.exp2(rng.integers(-20, 21, D).astype(np.float64))


def disjoint_rows(sizes):
    """Disjoint rows of the given sizes over sum(sizes) agents, in order: ``(rows, n)``."""
    n, at, lists = sum(sizes), 0, []
    for k in sizes:
        lists.append(range(at, at + k))
        at += k
    return M.pack(lists, n), n


def marginals_loop(mem, prob, n, descending=False):
    """(pi list, psum): per tile of 1024 rows every agent's sum from +0.0 in ascending row order, one add per
    holder; the tiles' sums added in ascending order from +0.0.  ``descending``: rows and tiles in the other
    order, for the order-sensitivity condition."""
    D = len(mem)
    tiles = [list(range(t0, min(t0 + TILE, D))) for t0 in range(0, D, TILE)]
    if descending:
        tiles = [tile[::-1] for tile in tiles[::-1]]
    pi, psum = [0.0] * n, 0.0
    for tile in tiles:
        part, ps = [0.0] * n, 0.0
        for d in tile:
            pd = float(prob[d])
            for i in mem[d]:
                part[i] = part[i] + pd
            ps = ps + pd
        for i in range(n):
            pi[i] = pi[i] + part[i]
        psum = psum + ps
    return pi, psum


def nash_loop(mem, n, rounds, mult=None, total=None, state=None, descending=False):
    """The contract over lists: dict(prob, scores, marginals, ratio, rounds, best_row, psum); ``state`` given:
    continued (a copy).  ``descending`` goes to the marginal sums."""
    D = len(mem)
    held = sorted({i for row in mem for i in row})
    m = float(len(held))

    def the_pass(prob):
        pi, psum = marginals_loop(mem, prob, n, descending)
        inv = [0.0] * n
        for i in held:
            inv[i] = 1.0 / pi[i]
        scores, at, value = [], None, None
        for d, row in enumerate(mem):
            s = 0.0
            for i in row:
                s = s + inv[i]
            scores.append(s)
            if at is None or s > value:
                at, value = d, s
        g = value / m
        return scores, pi, g * psum, at, psum

    if state is None:
        if not D:
            return {"prob": np.zeros(0), "scores": np.zeros(0), "marginals": np.zeros(n), "ratio": float("inf"),
                    "rounds": 0, "best_row": PRICE_NONE, "psum": 0.0}
        prob = [float(int(x)) / float(int(total)) for x in mult] if mult is not None else [1.0 / float(D)] * D
        scores, pi, ratio, at, psum = the_pass(prob)
        done = 0
    else:
        prob, scores, pi = ([float(x) for x in state[name]] for name in ("prob", "scores", "marginals"))
        ratio, done, at, psum = state["ratio"], state["rounds"], state["best_row"], state["psum"]
    for _ in range(rounds if D else 0):
        for d in range(D):
            g = scores[d] / m
            prob[d] = prob[d] * g
        scores, pi, ratio, at, psum = the_pass(prob)
        done += 1
    return {"prob": np.array(prob, np.float64), "scores": np.array(scores, np.float64),
            "marginals": np.array(pi, np.float64), "ratio": ratio, "rounds": done, "best_row": at, "psum": psum}


def same_state(got, want):
    """A stats.NashState against the loop's dict (or another NashState), bit for bit; the reason for a
    difference, or None."""
    if not isinstance(want, dict):
        want = {name: getattr(want, name) for name in want._fields}
    for name in ("prob", "scores", "marginals"):
        a, b = P.bits(getattr(got, name)), P.bits(want[name])
        if a.shape != b.shape or not np.array_equal(a, b):
            return name
    for name in ("ratio", "psum"):
        if P.bits1(getattr(got, name)) != P.bits1(want[name]):
            return name
    if (got.rounds, got.best_row) != (want["rounds"], want["best_row"]):
        return "rounds / best_row"
    return None


def exact(mem, n, prob):
    """From the floats p, in exact rational arithmetic: (pi, G, max G / m * sum p) with pi and G lists of
    Fractions."""
    p = [Fraction(float(x)) for x in prob]
    pi = [Fraction(0)] * n
    for d, row in enumerate(mem):
        for i in row:
            pi[i] += p[d]
    m = sum(1 for x in pi if x)
    G = [sum((1 / pi[i] for i in row), Fraction(0)) for row in mem]
    return pi, G, max(G) / m * sum(p, Fraction(0))


def geometric_mean(marginals, psum):
    """exp(fsum(log(pi / psum)) / m) over the agents with pi != 0."""
    v = [float(x) / float(psum) for x in marginals if x != 0.0]
    return math.exp(math.fsum(math.log(x) for x in v) / len(v))


@functools.lru_cache(maxsize=None)
def trajectory(name, start, rounds):
    """The mirror run one round at a time over a SHAPES table: the list of NashState after 0 .. ``rounds``
    rounds (each call continues the last)."""
    St = pkg("stats")
    rows, n = table(name)
    mult, total = mults(len(rows)) if start == "legacy" else (None, None)
    out = [St.rows_nash_host(rows, n, 0, mult, total)]
    for _ in range(rounds):
        out.append(St.rows_nash_host(rows, n, 1, state=out[-1]))
    return out


@functools.lru_cache(maxsize=None)
def mirror(name, start, rounds):
    """stats.rows_nash_host over a SHAPES table in one call, once."""
    rows, n = table(name)
    mult, total = mults(len(rows)) if start == "legacy" else (None, None)
    return pkg("stats").rows_nash_host(rows, n, rounds, mult, total)
