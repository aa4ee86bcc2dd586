"""Households for the register cells of tests/test_gpu_draw_matrix.py: the 70 solo8 / solo16 / lane recipes
(S = 613 from panel 2^32 - 300) with the same-address rings of tests/address_cases.ring_of, the C oracle's
draw of each with them (oracle.coracle.draw(..., addr_next=ring, ring_tally=...)), the household kernel each
cell runs under CSA_ADDRESS_BATCH, and the conditions a cell meets on the oracle alone before anything is
compared with it.  Shared by tests/test_households_host.py (no GPU) and tests/test_gpu_households_matrix.py.

Rings.  ring_of's recipe for 65 cells.  The five cells with n = 250 and k = 150 never finish with it (the
oracle ends at the attempt limit), so they take a lighter ring (light_ring_of): the same default_rng(7)
shuffle, the first 6 agents one household, the next 80 agents 40 couples, the rest alone:
  draw_solo_kernel<8, 4, 8, false>
  draw_solo_kernel<16, 4, 8, true>
  draw_solo_kernel<16, 4, 8, false>
  draw_lane_kernel<32, 4, 2, 8, true>
  draw_lane_kernel<32, 4, 2, 8, false>

Conditions (check_conditions, per cell, on the oracle's own output): rc == 0; no panel above 10 000 attempts;
at least 5 % of the panels restarted; at least 90 % differ from the cell's ring-free draw; where W > 1 at
least 100 same-address deletions fall in another word than their pick's; no accepted panel holds two members
of a ring.  Over the cells (check_ring_failures): the lane family and the solo families each show a cell with
at least 20 attempts that failed inside a same-address deletion.

The solo cell tuned for that last condition (SCARCE_SOLO): draw_solo_kernel<16, 4, 7, false>, which shows
17 such attempts with the matrix's recipe.  Its leading category's share of d0 goes from 0.7 to 0.45 (same
quotas, same pool seed), so d0 -- minimum 42 of k = 60 -- is scarce: 73 holders among the 165 agents,
and a household's deletion takes the feature below what it still needs in 24 attempts (0.41: 22, 0.40: 19,
0.37 and below: the oracle ends at the attempt limit).  The kernel the cell routes to is unchanged (F, n and
the quotas are).
"""
import collections
import functools
import os

import numpy as np

import address_cases as AC
from oracle import coracle
from test_gpu_draw_matrix import (BEGIN, CELLS, MAX_ATTEMPTS, S_SMALL, SEED, cell_S, oracle_instance,
                                  oracle_reference, recipe_of)

SCARCE_SOLO = "draw_solo_kernel<16, 4, 7, false>"
RETUNED = {SCARCE_SOLO: dict(dom=(0.45, (42, 42), (-120, 18)))}

REGISTER = [c._replace(**RETUNED.get(c.name, {})) for c in CELLS if c.family in ("solo8", "solo16", "lane")]
BY_NAME = {c.name: c for c in REGISTER}
LIGHT = ("draw_solo_kernel<8, 4, 8, false>", "draw_solo_kernel<16, 4, 8, true>", "draw_solo_kernel<16, 4, 8, false>",
         "draw_lane_kernel<32, 4, 2, 8, true>", "draw_lane_kernel<32, 4, 2, 8, false>")


def household_name(cell):
    """The household form a register cell runs under CSA_ADDRESS_BATCH: the cell's kernel without its slack
    planes parameter (the household forms are built for 8 planes only)."""
    head, args = cell.name.split("<")
    args = args.rstrip(">").split(", ")
    del args[-2]
    return "%s<%s>" % (head.replace("_kernel", "_hh_kernel"), ", ".join(args))


HOUSEHOLD_KERNELS = sorted({household_name(c) for c in REGISTER})


@functools.lru_cache(maxsize=None)
def light_ring_of(n):
    """(addr_next, household label) of the lighter recipe; both read-only."""
    order = np.random.default_rng(7).permutation(n)
    households = [order[:6]] + [order[6 + 2 * j:8 + 2 * j] for j in range(40)] + [order[86 + j:87 + j]
                                                                                  for j in range(n - 86)]
    nxt = AC.close_rings(n, households)
    label = np.zeros(n, np.int32)
    for h, members in enumerate(households):
        label[members] = h
    nxt.setflags(write=False)
    label.setflags(write=False)
    return nxt, label


def ring_for(cell):
    """(addr_next int32[n], household label int32[n]) of a register cell."""
    return light_ring_of(cell.n) if cell.name in LIGHT else AC.ring_of(cell.n)


@functools.lru_cache(maxsize=None)
def _reference(recipe, S, light):
    _, o = oracle_instance(recipe)
    ring, _ = light_ring_of(o.n) if light else AC.ring_of(o.n)
    rejects = np.zeros(S, np.uint32)
    tally = np.zeros(2, np.uint64)
    rc, panels, att, picks = coracle.draw(o, o.k, SEED, BEGIN, S, max_attempts=MAX_ATTEMPTS, want_picks=True,
                                          rejects=rejects, threads=min(16, os.cpu_count() or 1), addr_next=ring,
                                          ring_tally=tally)
    for a in (panels, att, picks, rejects):
        a.setflags(write=False)
    stats = {"attempts": int(att.sum()), "rejections": int(rejects.sum()),
             "selection_errors": int(att.sum()) - S - int(rejects.sum())}
    return AC.AddressReference(rc, panels, att, picks, rejects, stats, BEGIN, 2 ** 32 - BEGIN, int(tally[0]),
                               int(tally[1]))


def reference_of(cell):
    """The C oracle's draw of the cell's batch with the cell's rings, computed once, read-only."""
    assert cell_S(cell) == S_SMALL
    return _reference(recipe_of(cell), S_SMALL, cell.name in LIGHT)


def base_of(cell):
    """The cell's ring-free draw."""
    return oracle_reference(recipe_of(cell), S_SMALL)


Figures = collections.namedtuple("Figures", "panels differ restarted most_attempts attempts ring_failures cross_word")


def figures(cell):
    ref, base = reference_of(cell), base_of(cell)
    return Figures(len(ref.attempts), int((ref.panels != base.panels).any(axis=1).sum()),
                   int((ref.attempts > 1).sum()), int(ref.attempts.max()), ref.stats["attempts"], ref.ring_failures,
                   ref.cross_word)


def check_conditions(cell):
    """The per-cell conditions of the module docstring; returns the cell's reference."""
    ref, fig = reference_of(cell), figures(cell)
    S = fig.panels
    print("%s with rings: %s %s" % (cell.name, fig, ref.stats))
    assert ref.rc == 0
    assert fig.most_attempts <= 10000
    assert fig.restarted * 20 >= S, "fewer than 5 %% of the panels restarted (%d of %d)" % (fig.restarted, S)
    assert fig.differ * 10 >= S * 9, "fewer than 90 %% of the panels differ from the ring-free draw"
    assert 0 < ref.carry < S - 1 and ref.carry % 64          # the batch carries the panel index mid-block
    if (cell.n + 63) // 64 > 1:
        assert fig.cross_word >= 100
    _, label = ring_for(cell)
    assert (ref.picks >= 0).all()
    houses = np.sort(label[ref.picks], axis=1)                # [S, k] household of every pick
    assert (houses[:, 1:] != houses[:, :-1]).all(), "a panel holds two members of one household"
    return ref


def check_ring_failures():
    """Over the cells: the deferred failure test has something to agree with, in both kernels."""
    for families in (("lane",), ("solo8", "solo16")):
        best = max(reference_of(c).ring_failures for c in REGISTER if c.family in families)
        assert best >= 20, (families, best)
