"""Households for the GENERAL cells of tests/test_gpu_draw_matrix.py: the same-address rings that
tests/test_oracle_address.py (no GPU) and tests/test_gpu_address_matrix.py share, the C oracle's draw of
each cell with them, and the conditions an instance has to meet before anything is compared with it.

The ring recipe (ring_of): the agents shuffled by default_rng(7); the first BIG of them are one
household (70 members where n > 1000: more than one 64-person word and many lanes; 6 at n = 165, where
70 would drive draw_kernel<64, 2, 1, true> to about a million attempts); the rest fall into households
of 1 to 4 members (40 / 30 / 20 / 10 %).  A household's members are sorted ascending and closed into a
ring (legacy.address_rings' order); a lone agent points to itself.

Conditions (check_conditions, per cell, on the oracle's own output):
  * rc == 0, no panel above 10 000 attempts, the cell's attempts <= 100 000 (the ring-free matrix's
    largest cell runs 49 960: a cell stays at seconds);
  * at least 5 % of the panels restarted, at least 90 % differ from the cell's ring-free draw;
  * W > 1: at least 100 same-address deletions fall in another word than their pick's;
  * no accepted panel holds two members of one ring (what the feature exists for).
Over the cells (check_ring_failures): at least two show >= 20 attempts that a same-address deletion
failed by emptying a feature below its minimum, at least one of them with FPL > 1.
"""
import collections
import functools
import os

import numpy as np

from oracle import coracle
from test_gpu_draw_matrix import (BEGIN, BEGIN_LARGE, CELLS, MAX_ATTEMPTS, S_SMALL, SEED, UNLAUNCHABLE, cell_S,
                                  oracle_instance, oracle_reference, recipe_of)

GENERAL = [c for c in CELLS if c.family == "g64-general"]
LAUNCHABLE = [c for c in GENERAL if c.name not in UNLAUNCHABLE]
REFUSED = [c for c in GENERAL if c.name in UNLAUNCHABLE]
HOUSE_SHARES = (0.4, 0.3, 0.2, 0.1)    # households of 1, 2, 3, 4 members


def fpl_wpl(cell):
    """(FPL, WPL) of a draw_kernel<64, FPL, WPL, true> cell."""
    fpl, wpl = cell.name[len("draw_kernel<64, "):].split(", ")[:2]
    return int(fpl), int(wpl)


def close_rings(n, households):
    """addr_next int32[n]: every household sorted ascending and closed into a ring; agents in no household
    point to themselves."""
    nxt = np.arange(n, dtype=np.int32)
    for members in households:
        members = sorted(int(p) for p in members)
        for j, p in enumerate(members):
            nxt[p] = members[(j + 1) % len(members)]
    return nxt


@functools.lru_cache(maxsize=None)
def ring_of(n):
    """(addr_next int32[n], household label int32[n]) of the recipe; both read-only."""
    rng = np.random.default_rng(7)
    order = rng.permutation(n)
    big = 70 if n > 1000 else 6
    households, at = [order[:big]], big
    sizes = 1 + rng.choice(4, size=n, p=HOUSE_SHARES)
    for size in sizes:
        if at >= n:
            break
        households.append(order[at:at + size])
        at += size
    nxt = close_rings(n, households)
    label = np.zeros(n, np.int32)
    for h, members in enumerate(households):
        label[members] = h
    nxt.setflags(write=False)
    label.setflags(write=False)
    return nxt, label


AddressReference = collections.namedtuple(
    "AddressReference", "rc panels attempts picks rejects stats begin carry ring_failures cross_word")


@functools.lru_cache(maxsize=None)
def address_reference(recipe, S):
    """The C oracle's draw of a recipe's batch with the recipe's rings, computed once, read-only."""
    _, o = oracle_instance(recipe)
    ring, _ = ring_of(o.n)
    rejects = np.zeros(S, np.uint32)
    tally = np.zeros(2, np.uint64)
    begin = BEGIN if S == S_SMALL else BEGIN_LARGE
    rc, panels, att, picks = coracle.draw(o, o.k, SEED, begin, S, max_attempts=MAX_ATTEMPTS, want_picks=True,
                                          rejects=rejects, threads=min(16, os.cpu_count() or 1), addr_next=ring,
                                          ring_tally=tally)
    for a in (panels, att, picks, rejects):
        a.setflags(write=False)
    stats = {"attempts": int(att.sum()), "rejections": int(rejects.sum()),
             "selection_errors": int(att.sum()) - S - int(rejects.sum())}
    return AddressReference(rc, panels, att, picks, rejects, stats, begin, 2 ** 32 - begin, int(tally[0]),
                            int(tally[1]))


def reference_of(cell):
    return address_reference(recipe_of(cell), cell_S(cell))


def figures(cell):
    """The cell's figures on the oracle alone."""
    ref, base = reference_of(cell), oracle_reference(recipe_of(cell), cell_S(cell))
    return {"panels": len(ref.attempts),
            "differ": int((ref.panels != base.panels).any(axis=1).sum()),
            "restarted": int((ref.attempts > 1).sum()),
            "most_attempts": int(ref.attempts.max()),
            "attempts": ref.stats["attempts"],
            "ring_failures": ref.ring_failures,
            "cross_word": ref.cross_word}


def check_conditions(cell):
    """The per-cell conditions of the module docstring; returns the cell's reference."""
    ref, fig = reference_of(cell), figures(cell)
    S = fig["panels"]
    print("%s with rings: %s %s" % (cell.name, fig, ref.stats))
    assert ref.rc == 0
    assert fig["most_attempts"] <= 10000
    assert fig["attempts"] <= 100000
    assert fig["restarted"] * 20 >= S, "fewer than 5 %% of the panels restarted (%d of %d)" % (fig["restarted"], S)
    assert fig["differ"] * 10 >= S * 9, "fewer than 90 %% of the panels differ from the ring-free draw"
    assert 0 < ref.carry < S - 1 and ref.carry % 64          # the batch carries the panel index mid-block
    if (cell.n + 63) // 64 > 1:
        assert fig["cross_word"] >= 100
    _, label = ring_of(cell.n)
    houses = label[ref.picks]                                 # [S, k] household of every pick
    assert (ref.picks >= 0).all()
    assert all(len(set(row)) == cell.k for row in houses.tolist()), "a panel holds two members of one household"
    return ref


def check_ring_failures():
    """The condition over the cells: the deferred failure test has something to agree with."""
    hit = [c for c in LAUNCHABLE if reference_of(c).ring_failures >= 20]
    assert len(hit) >= 2 and any(fpl_wpl(c)[0] > 1 for c in hit), [(c.name, reference_of(c).ring_failures)
                                                                   for c in LAUNCHABLE]
