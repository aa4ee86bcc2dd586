"""Every draw-kernel instantiation the library can launch, each against the C oracle.

``csa_draw_kernel_list`` names what the dispatcher (pick_draw_config) can resolve: the rows of the table
of built kernels it looks its kernel up in (kDrawKernels, csrc/draw_dispatch.inc).  CELLS holds one
synthetic instance per name, the smallest that routes there, and test_matrix_covers_every_built_kernel
(no GPU) fails when the two sets differ.  Each cell then checks, bit for bit against
``oracle.coracle.draw`` on the same instance:

  * csa_draw_kernel_name (for a GENERAL cell: the batch name under CSA_DRAW_KERNEL=64, which differs
    from the cell's only in draw_kernel's GENERAL parameter -- the name entry never reports GENERAL);
  * csa_legacy_sample: panels, attempts per panel, attempts / rejections / selection_errors;
  * solo, lane, wide: csa_draw_picks_async picks in pick order;
  * solo, lane: DevicePipeline.draw_xt -- panels, hashes, attempts, the fused XT (buffers pre-filled
    with -1) and the per-person counts;
  * GENERAL cells: csa_legacy_find picks in pick order, attempts and statistics;
  * the panel index CSA_E_ATTEMPT_LIMIT reports (the status block's two index words) for the one panel
    past 2^32 that an attempt limit one short of its need stops.

Batch: S = 613 panels (9 blocks of 64 and a ragged 37) from panel 2^32 - 300, so every batch carries
the panel index into its high word in the middle of a block; S = 237 for the pools of more than 128
words, from panel 2^32 - 100 (from 2^32 - 300 they would end before the carry).  Before a cell compares
anything it asserts on the oracle's own output that rc == 0, that at least 5 % of the panels restarted
and that no panel took more than 10 000 attempts; per family one cell (RESTART_CELLS) must show at least
20 rejections and 20 SelectionErrors.

Recipes.  F: a leading two-feature category "d" with explicit quotas (where the cell needs one) plus
random categories (shares ~ Dirichlet(2), quotas floor(lo k p) / ceil(hi k p)) put F in the band; n puts
W = ceil(n / 64) just past the previous bucket's edge with a ragged last word (W = 3, 5, 9, 17, 29 for
WN = 4, 8, 16, 28, 32; W = 4 and 8 where a cell draws k = 150); the largest maximum selects the slack
planes NP (< 32: 5, < 128: 7, else 8); a minimum above 127 selects the 16-bit keys (K8 = false).
K8 = false with NP = 5 or 7 cannot be had that way (a minimum above 127 has a maximum above 127): the
dispatcher also takes the 16-bit keys when max - min > 127, so those cells give d1 a minimum of -120,
which the reference arithmetic treats as any other minimum that is already met.

Exempt from the 5 % restart floor (EXEMPT): none.

Cells the dispatcher resolves but launch_draw refuses (UNLAUNCHABLE: their feature rows alone, 64 FPL x
(64 WPL + 1) words, exceed 160 KiB of LDS); asserted to return CSA_E_UNSUPPORTED, launch nothing and
leave the status block untouched:
  draw_kernel<64, 2, 4, false>
  draw_kernel<64, 4, 2, false>
  draw_kernel<64, 4, 4, false>
  draw_kernel<64, 2, 4, true>
  draw_kernel<64, 4, 2, true>
  draw_kernel<64, 4, 4, true>
"""
import collections
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import pkg
from oracle import coracle
from oracle.legacy_oracle import OracleInstance

S_SMALL, S_LARGE = 613, 200 + 37
BEGIN = 2 ** 32 - 300          # S_SMALL: panel 2^32 is row 300 (4 blocks of 64 and 44)
BEGIN_LARGE = 2 ** 32 - 100    # S_LARGE: row 100 (from 2^32 - 300 the 237 panels would end before the carry)
SEED = 20240611
MAX_ATTEMPTS = 100000

# name: the instantiation; family: solo8 / solo16 / lane / wide / g16 / g64 / g64-general;
# dom: None or (share of d0, (min, max) of d0, (min, max) of d1); cats: features per random category;
# via: "default" routing, a CSA_DRAW_KERNEL force ("wide", "16", "64") or "find" (csa_legacy_find)
Cell = collections.namedtuple("Cell", "name family dom cats n k lo hi seed via")

WN_N = {4: 64 * 2 + 37, 8: 64 * 4 + 37, 16: 64 * 8 + 37, 28: 64 * 16 + 37, 32: 64 * 28 + 37}
# the K8 = false, NP = 8 cells draw k = 150: the two smallest buckets need more people than that
WN_N_BIG = {**WN_N, 4: 64 * 3 + 58, 8: 64 * 7 + 37}

# (NP, K8) -> (k, dom) of a register-kernel cell
REG_VARIANTS = {
    (5, True): (20, None),
    (7, True): (60, (0.7, (42, 42), (18, 18))),
    (8, True): (150, (0.86, (127, 131), (19, 23))),
    (8, False): (150, (0.86, (131, 131), (19, 19))),
    (5, False): (20, (0.5, (10, 10), (-120, 10))),
    (7, False): (60, (0.7, (42, 42), (-120, 18))),
}

# per cell, the recipe fields tuned on the CPU with the C oracle until the instance conditions hold (cells
# not listed: lo = hi = 1.0, pool seed 1)
TUNED = {
    # the restart cells of the two solo families: a scarce d1 (5 holders for a quota of 4 to 5) fails
    # with SelectionErrors, the tight random categories with rejections; 16 features in 4 categories
    "draw_solo_kernel<8, 4, 8, true>": dict(dom=(1 - 5 / 165, (15, 16), (4, 5)), seed=4),
    "draw_solo_kernel<16, 4, 5, true>": dict(cats=(4, 4, 4, 4), k=16, seed=4),
    "draw_solo_kernel<8, 8, 8, true>": dict(seed=4),
    "draw_solo_kernel<8, 16, 8, true>": dict(seed=4),
    "draw_solo_kernel<8, 28, 8, true>": dict(seed=4),
    "draw_solo_kernel<8, 32, 8, true>": dict(seed=4),
    "draw_solo_kernel<8, 4, 8, false>": dict(seed=2),
    "draw_solo_kernel<8, 28, 8, false>": dict(seed=2),
    "draw_solo_kernel<8, 32, 8, false>": dict(seed=2),
    "draw_kernel<64, 2, 1, false>": dict(lo=0.96, hi=1.04, seed=4),
    "draw_kernel<64, 2, 1, true>": dict(lo=0.96, hi=1.04, seed=4),
    "draw_kernel<64, 2, 2, false>": dict(seed=4),
    "draw_kernel<64, 2, 2, true>": dict(seed=4),
    "draw_kernel<64, 4, 1, false>": dict(lo=0.7, hi=1.4),     # 17 tight categories never finish
    "draw_kernel<64, 4, 1, true>": dict(lo=0.7, hi=1.4),
}

# cells exempt from the 5 % restart floor (at most 10 % of the cells; named in the docstring)
EXEMPT = ()

# cells launch_draw refuses (named in the docstring)
UNLAUNCHABLE = (
    "draw_kernel<64, 2, 4, false>", "draw_kernel<64, 4, 2, false>", "draw_kernel<64, 4, 4, false>",
    "draw_kernel<64, 2, 4, true>", "draw_kernel<64, 4, 2, true>", "draw_kernel<64, 4, 4, true>",
)

# per family, the cell whose oracle run must show >= 20 rejections and >= 20 SelectionErrors
RESTART_CELLS = {
    "solo8": "draw_solo_kernel<8, 4, 8, true>",
    "solo16": "draw_solo_kernel<16, 4, 5, true>",
    "lane": "draw_lane_kernel<32, 4, 2, 8, true>",
    "wide": "draw_wide_kernel<8, 5, 4>",
    "g16": "draw_kernel<16, 4, 1, false>",
    "g64": "draw_kernel<64, 2, 2, false>",
    "g64-general": "draw_kernel<64, 2, 2, true>",
}


def _bool(b):
    return "true" if b else "false"


def _cell(name, family, dom, cats, n, k, via):
    cell = Cell(name, family, dom, tuple(cats), n, k, 1.0, 1.0, 1, via)
    return cell._replace(**TUNED.get(name, {}))


def _cells():
    out = []
    # draw_solo_kernel<8, WN, 8, K8>: F = 8 (6 at K8 = true); no slack planes at FN = 8
    for wn in (4, 8, 16, 28, 32):
        out.append(_cell("draw_solo_kernel<8, %d, 8, true>" % wn, "solo8", None, (3, 3), WN_N[wn], 20, "default"))
        k, dom = REG_VARIANTS[(8, False)]
        out.append(_cell("draw_solo_kernel<8, %d, 8, false>" % wn, "solo8", dom, (3, 3), WN_N_BIG[wn], k, "default"))
    # draw_solo_kernel<16, WN, NP, K8> (F = 12 / 14) and draw_lane_kernel<32, WN, WN / 2, NP, K8> (F = 20 / 22)
    for wn in (4, 8, 16, 28, 32):
        for (np_, k8), (k, dom) in REG_VARIANTS.items():
            n = (WN_N_BIG if k == 150 else WN_N)[wn]
            out.append(_cell("draw_solo_kernel<16, %d, %d, %s>" % (wn, np_, _bool(k8)), "solo16", dom, (4, 4, 4),
                             n, k, "default"))
            out.append(_cell("draw_lane_kernel<32, %d, %d, %d, %s>" % (wn, wn // 2, np_, _bool(k8)), "lane", dom,
                             (5, 5, 5, 5), n, k, "default"))
    # draw_wide_kernel<8, FPL, WPL>: FPL = 2 / 4 / 5 / 8 at F = 12 / 20 / 35 / 42, WPL = 4 / 8 / 16 at W = 5 /
    # 33 / 65; the register kernels take F <= 32 at W <= 32 by default, so those cells are forced
    for fpl, cats in ((2, (4, 4, 4)), (4, (5, 5, 5, 5)), (5, (7,) * 5), (8, (7,) * 6)):
        for wpl, n in ((4, 64 * 4 + 37), (8, 64 * 32 + 37), (16, 64 * 64 + 37)):
            via = "wide" if fpl <= 4 and wpl == 4 else "default"
            out.append(_cell("draw_wide_kernel<8, %d, %d>" % (fpl, wpl), "wide", None, cats, n, 20, via))
    # draw_kernel<16, FPL, WPL, false>: FPL = 1 / 2 / 4 at F = 12 / 20 / 35, WPL = 1 .. 16 at W = 3, 17, 33, 65, 129
    for fpl, cats in ((1, (4, 4, 4)), (2, (5, 5, 5, 5)), (4, (7,) * 5)):
        for wpl, n in ((1, 64 * 2 + 37), (2, 64 * 16 + 37), (4, 64 * 32 + 37), (8, 64 * 64 + 37), (16, 64 * 128 + 37)):
            out.append(_cell("draw_kernel<16, %d, %d, false>" % (fpl, wpl), "g16", None, cats, n, 20, "16"))
    # draw_kernel<64, FPL, WPL, GEN>: FPL = 1 / 2 / 4 at F = 20 / 72 / 136, WPL = 1 / 2 / 4 at W = 3 / 65 / 129
    for gen in (False, True):
        for fpl, cats in ((1, (5, 5, 5, 5)), (2, (8,) * 9), (4, (8,) * 17)):
            for wpl, n in ((1, 64 * 2 + 37), (2, 64 * 64 + 37), (4, 64 * 128 + 37)):
                via = "find" if gen else "default" if fpl > 1 else "64"   # F <= 64 takes G = 16 unforced
                out.append(_cell("draw_kernel<64, %d, %d, %s>" % (fpl, wpl, _bool(gen)),
                                 "g64-general" if gen else "g64", None, cats, n, 20, via))
    return out


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
FAMILIES = ("solo8", "solo16", "lane", "wide", "g16", "g64", "g64-general")


def cell_S(cell):
    return S_LARGE if cell.n > 128 * 64 else S_SMALL


def build_pool(cell):
    """(categories, fmin, fmax, fcat, person_feat int array [n, C]) of a cell's recipe."""
    rng = np.random.default_rng(cell.seed)
    k, n = cell.k, cell.n
    specs = []   # per category: (shares, minima, maxima)
    if cell.dom:
        share, q0, q1 = cell.dom
        specs.append((np.array([share, 1.0 - share]), [q0[0], q1[0]], [q0[1], q1[1]]))
    for nf in cell.cats:
        p = rng.dirichlet(np.full(nf, 2.0))
        specs.append((p, [int(np.floor(cell.lo * k * x)) for x in p], [int(np.ceil(cell.hi * k * x)) for x in p]))
    cats, fmin, fmax, fcat, cols, base = {}, [], [], [], [], 0
    for c, (p, mins, maxs) in enumerate(specs):
        cname = "d" if cell.dom and c == 0 else "c%d" % c
        cats[cname] = {"f%d" % j: {"min": mins[j], "max": maxs[j]} for j in range(len(p))}
        fmin += mins
        fmax += maxs
        fcat += [c] * len(p)
        cols.append(base + rng.choice(len(p), size=n, p=p))
        base += len(p)
    return cats, fmin, fmax, fcat, np.stack(cols, axis=1)


@functools.lru_cache(maxsize=None)
def oracle_instance(recipe):
    """(categories, OracleInstance) of a recipe (a Cell without its name, family and route)."""
    cell = Cell("", "", *recipe, "")
    cats, fmin, fmax, fcat, pf = build_pool(cell)
    names = [(c, f) for c in cats for f in cats[c]]
    o = OracleInstance(k=cell.k, cat_names=list(cats), feat_names=names, fmin=fmin, fmax=fmax, fcat=fcat,
                       person_feat=pf.tolist())
    return cats, o


Reference = collections.namedtuple("Reference", "rc panels attempts picks rejects stats begin carry")


@functools.lru_cache(maxsize=None)
def oracle_reference(recipe, S):
    """The C oracle's draw of a recipe's batch, computed once and shared read-only."""
    _, o = oracle_instance(recipe)
    rejects = np.zeros(S, np.uint32)
    begin = BEGIN if S == S_SMALL else BEGIN_LARGE
    rc, panels, att, picks = coracle.draw(o, o.k, SEED, begin, S, max_attempts=MAX_ATTEMPTS, want_picks=True,
                                          rejects=rejects, threads=min(16, os.cpu_count() or 1))
    for a in (panels, att, picks, rejects):
        a.setflags(write=False)
    stats = {"attempts": int(att.sum()), "rejections": int(rejects.sum()),
             "selection_errors": int(att.sum()) - S - int(rejects.sum())}
    return Reference(rc, panels, att, picks, rejects, stats, begin, 2 ** 32 - begin)


def recipe_of(cell):
    return tuple(cell[2:9])


def check_instance_conditions(cell, ref):
    """The issue's conditions on the oracle's own output: an instance that never restarts tests half
    a kernel."""
    S = len(ref.attempts)
    assert ref.rc == 0
    restarted = int((ref.attempts > 1).sum())
    print("%s: %d of %d panels restarted, most attempts %d, %s" % (cell.name, restarted, S, ref.attempts.max(),
                                                                   ref.stats))
    assert ref.attempts.max() <= 10000
    if cell.name not in EXEMPT:
        assert restarted * 20 >= S, "fewer than 5 %% of the panels restarted (%d of %d)" % (restarted, S)
    assert 0 < ref.carry < S - 1 and ref.carry % 64 and (ref.attempts[ref.carry:] > 1).any()   # _check_status_panel
    if RESTART_CELLS.get(cell.family) == cell.name:
        assert ref.stats["rejections"] >= 20 and ref.stats["selection_errors"] >= 20, ref.stats


def batch_name(cell):
    """What csa_draw_kernel_name reports where the cell's kernel runs (it never reports GENERAL)."""
    return cell.name.replace("true>", "false>") if cell.via == "find" else cell.name


# ---- completeness (no GPU) --------------------------------------------------------------------------

def test_matrix_covers_every_built_kernel():
    """CELLS names exactly the instantiations the dispatcher can resolve: a new instantiation without a
    cell, or a cell whose instantiation is gone, fails here."""
    N = pkg("_native")
    built = N.draw_kernel_list()
    assert len(built) == len(set(built)) and len(built) >= 100
    names = [c.name for c in CELLS]
    assert len(names) == len(set(names))
    assert set(names) == set(built), (sorted(set(built) - set(names)), sorted(set(names) - set(built)))
    assert set(EXEMPT) <= set(names) and len(EXEMPT) * 10 <= len(names)
    assert set(UNLAUNCHABLE) <= set(names) and not set(UNLAUNCHABLE) & set(EXEMPT)
    assert sorted(RESTART_CELLS) == sorted(FAMILIES)
    assert all(BY_NAME[n].family == f and n not in UNLAUNCHABLE for f, n in RESTART_CELLS.items())
    for n in list(EXEMPT) + list(UNLAUNCHABLE):
        assert "  " + n + "\n" in __doc__


def test_cells_meet_the_instance_conditions():
    """Every launchable cell's recipe, on the oracle alone: restarts, attempt ceiling and the per-family
    rejection / SelectionError floors hold before any GPU is asked (the cells assert them again)."""
    for cell in CELLS:
        if cell.name not in UNLAUNCHABLE:
            check_instance_conditions(cell, oracle_reference(recipe_of(cell), cell_S(cell)))


def test_kernel_list_reports_needed_size():
    N = pkg("_native")
    need = len("\n".join(N.draw_kernel_list())) + 2
    small = ctypes.create_string_buffer(need - 1)
    assert N.lib().csa_draw_kernel_list(small, need - 1) == N.CSA_E_INVALID
    assert str(need) in N.last_error()
    assert N.lib().csa_draw_kernel_list(None, 0) == N.CSA_E_INVALID
    exact = ctypes.create_string_buffer(need)
    assert N.lib().csa_draw_kernel_list(exact, need) == N.CSA_OK
    assert exact.value.decode().splitlines() == N.draw_kernel_list()


def test_oracle_carries_the_panel_index():
    """The reference of every cell is itself checked where the cells put their batch: across panel 2^32
    the C oracle agrees with the pure-Python oracle, whose integers have no width to slip on."""
    from oracle.legacy_oracle import PhiloxRng, legacy_find
    cell = BY_NAME["draw_solo_kernel<8, 4, 8, true>"]
    _, o = oracle_instance(recipe_of(cell))
    ref = oracle_reference(recipe_of(cell), cell_S(cell))
    for i in (0, 298, 299, 300, 301, 612):
        picks, attempts = legacy_find(o, o.k, PhiloxRng(SEED), BEGIN + i)
        assert attempts == ref.attempts[i] and list(picks) == ref.picks[i].tolist()
    # and the two sides of the carry are different streams
    lo = coracle.draw(o, o.k, SEED, BEGIN + 300 - 2 ** 32, 8, max_attempts=MAX_ATTEMPTS, want_picks=True)
    assert not np.array_equal(lo[3], ref.picks[300:308])


# ---- the cells (GPU) --------------------------------------------------------------------------------

@pytest.fixture
def draw_group():
    """Force a batch draw layout (CSA_DRAW_KERNEL), restoring the old value."""
    old = os.environ.get("CSA_DRAW_KERNEL")

    def set_layout(g):
        if g is None:
            os.environ.pop("CSA_DRAW_KERNEL", None)
        else:
            os.environ["CSA_DRAW_KERNEL"] = str(g)
    yield set_layout
    if old is None:
        os.environ.pop("CSA_DRAW_KERNEL", None)
    else:
        os.environ["CSA_DRAW_KERNEL"] = old


SEEN = {}   # cell name -> the csa_draw_kernel_name observed where the cell ran


def _kernel_name(enc, k):
    N = pkg("_native")
    buf = ctypes.create_string_buffer(128)
    N.check(N.lib().csa_draw_kernel_name(enc.handle, k, buf, 128))
    return buf.value.decode()


def _encode(cell):
    cats, o = oracle_instance(recipe_of(cell))
    names = [(c, f) for c in cats for f in cats[c]]
    agents = {i: {names[g][0]: names[g][1] for g in row} for i, row in enumerate(o.person_feat)}
    return pkg().encode(cats, agents), o


def _xt_reference(panels, n, npad):
    """panels uint64 [S, W] -> XT as uint32 [nblk, 2, npad] (include/csa_legacy.h: plane h of block b holds
    panels 64 b + 32 h .., bit j = panel 64 b + 32 h + j; zero past S and past n)."""
    S, W = panels.shape
    nblk = (S + 63) // 64
    bits = np.unpackbits(np.ascontiguousarray(panels).view(np.uint8).reshape(S, W * 8), axis=1,
                         bitorder="little")[:, :n]
    B = np.zeros((nblk * 64, npad), dtype=np.uint8)
    B[:S, :n] = bits
    B = B.reshape(nblk, 2, 32, npad)
    xt = np.packbits(B, axis=2, bitorder="little").reshape(nblk, 2, 4, npad)
    return np.ascontiguousarray(xt.transpose(0, 1, 3, 2)).view(np.uint32).reshape(nblk, 2, npad)


def _same(got, want, what):
    """Bit-exact, one row per panel; a mismatch names the first panel instead of printing the arrays."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
        raise AssertionError("%s differ from the oracle in %d of %d rows, first at row %d"
                             % (what, len(bad), len(want), bad[0]))


def _check_sample(enc, ref, k, S):
    N, A = pkg("_native"), pkg("analysis")
    panels = np.zeros((S, enc.W), np.uint64)
    attempts = np.zeros(S, np.uint32)
    A.draw_stats(enc, reset=True)
    N.check(N.lib().csa_legacy_sample(enc.handle, k, SEED, ref.begin, S, N.CSA_WANT_PANELS, MAX_ATTEMPTS,
                                      N.ptr(panels), None, None, None, N.ptr(attempts)))
    stats = A.draw_stats(enc)
    _same(attempts, ref.attempts, "csa_legacy_sample attempts")
    _same(panels, ref.panels, "csa_legacy_sample panels")
    assert stats == ref.stats


def _check_picks(enc, ref, k, S):
    import torch
    N, A = pkg("_native"), pkg("analysis")
    assert N.lib().csa_draw_picks_supported(enc.handle, k) == 1
    kp = int(N.lib().csa_picks_stride(k))
    picks = torch.full((S * kp,), -1, dtype=torch.int16, device="cuda")
    att = torch.zeros(S, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    A.draw_stats(enc, reset=True)
    N.check(N.lib().csa_draw_picks_async(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(picks), N.ptr(att),
                                         N.ptr(status), None))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    _same(att.cpu().numpy().view(np.uint32), ref.attempts, "csa_draw_picks_async attempts")
    got = picks.cpu().numpy().view(np.uint16).astype(np.int32).reshape(S, kp)[:, :k]
    _same(got, ref.picks, "csa_draw_picks_async picks")
    assert A.draw_stats(enc) == ref.stats


def _check_fused_xt(enc, ref, k, S):
    import torch
    A, D, Dv = pkg("analysis"), pkg("distributed"), pkg("device")
    W, nblk = enc.W, (S + 63) // 64
    pipe = Dv.DevicePipeline(enc, k, S, want_attempts=True)
    pipe.reset()
    for t in (pipe.xt, pipe.panels, pipe.hashes, pipe.attempts):
        t.fill_(-1)                                   # every word the draw owns must be written
    A.draw_stats(enc, reset=True)
    assert pipe.draw_xt(SEED, ref.begin, S, max_attempts=MAX_ATTEMPTS)
    pipe.pair_counts(S, overwrite=True, alone=True)
    pipe.counts_from_pairs()
    torch.cuda.synchronize()
    assert pipe.status.tolist() == [0, 0, 0, 0]
    _same(pipe.attempts[:S].cpu().numpy().view(np.uint32), ref.attempts, "draw_xt attempts")
    _same(pipe.panels[: S * W].cpu().numpy().view(np.uint64).reshape(S, W), ref.panels, "draw_xt panels")
    _same(pipe.hashes[: 2 * S].cpu().numpy().view(np.uint64).reshape(S, 2), D.panel_hashes(ref.panels),
          "draw_xt hashes")
    xt = pipe.xt[: nblk * pipe.npad].cpu().numpy().view(np.uint32).reshape(nblk, 2, pipe.npad)
    assert np.array_equal(xt, _xt_reference(ref.panels, enc.n, pipe.npad))
    assert np.array_equal(pipe.counts.cpu().numpy(), coracle.counts(ref.panels, enc.n))
    assert A.draw_stats(enc) == ref.stats


def _check_find(enc, ref, k, S):
    N, A = pkg("_native"), pkg("analysis")
    picks = np.full((S, k), -1, np.int32)
    attempts = np.zeros(S, np.uint32)
    A.draw_stats(enc, reset=True)
    N.check(N.lib().csa_legacy_find(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(picks), N.ptr(attempts)))
    stats = A.draw_stats(enc)
    _same(attempts, ref.attempts, "csa_legacy_find attempts")
    _same(picks, ref.picks, "csa_legacy_find picks")
    assert stats == ref.stats


def _check_status_panel(enc, ref, cell):
    """The status block carries the whole panel index: from panel 2^32 on, draw up to and including the
    first panel the oracle restarted, with an attempt limit one short of what that panel needs -- every
    panel before it is accepted at its first attempt, so exactly that one raises CSA_E_ATTEMPT_LIMIT."""
    N = pkg("_native")
    first = ref.carry + int(np.flatnonzero(ref.attempts[ref.carry:] > 1)[0])
    S, limit = first - ref.carry + 1, int(ref.attempts[first]) - 1
    if cell.via == "find":
        picks = np.full((S, cell.k), -1, np.int32)
        rc = N.lib().csa_legacy_find(enc.handle, cell.k, SEED, 2 ** 32, S, limit, N.ptr(picks), None)
    else:
        panels = np.zeros((S, enc.W), np.uint64)
        rc = N.lib().csa_legacy_sample(enc.handle, cell.k, SEED, 2 ** 32, S, N.CSA_WANT_PANELS, limit,
                                       N.ptr(panels), None, None, None, None)
    assert rc == N.CSA_E_ATTEMPT_LIMIT
    assert N.last_error().startswith("panel %d:" % (ref.begin + first)), N.last_error()


def _check_unlaunchable(enc, cell, S):
    """launch_draw refuses the cell: CSA_E_UNSUPPORTED from every entry, nothing launched, the status
    block as the caller left it."""
    import torch
    N = pkg("_native")
    L = N.lib()
    status = torch.tensor([0x5A5A5A5A, 1, 2, 3], dtype=torch.int32, device="cuda")
    panels = torch.full((S * enc.W,), -1, dtype=torch.int64, device="cuda")
    if cell.via == "find":
        picks = np.full((S, cell.k), -1, np.int32)
        assert L.csa_legacy_find(enc.handle, cell.k, SEED, BEGIN, S, MAX_ATTEMPTS, N.ptr(picks), None) == \
            N.CSA_E_UNSUPPORTED
        assert "LDS" in N.last_error()
        assert np.all(picks == -1)
        dpicks = torch.full((S * cell.k,), -1, dtype=torch.int32, device="cuda")
        rc = L.csa_draw_async(enc.handle, cell.k, SEED, BEGIN, S, MAX_ATTEMPTS, N.ptr(panels), None, None,
                              N.ptr(dpicks), N.ptr(status), None)
    else:
        host = np.zeros((S, enc.W), np.uint64)
        assert L.csa_legacy_sample(enc.handle, cell.k, SEED, BEGIN, S, N.CSA_WANT_PANELS, MAX_ATTEMPTS,
                                   N.ptr(host), None, None, None, None) == N.CSA_E_UNSUPPORTED
        assert "LDS" in N.last_error()
        rc = L.csa_draw_async(enc.handle, cell.k, SEED, BEGIN, S, MAX_ATTEMPTS, N.ptr(panels), None, None,
                              None, N.ptr(status), None)
    assert rc == N.CSA_E_UNSUPPORTED and "LDS" in N.last_error()
    torch.cuda.synchronize()
    assert status.tolist() == [0x5A5A5A5A, 1, 2, 3]
    assert bool((panels == -1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_cell_matches_oracle(gpu_available, draw_group, cell):
    S = cell_S(cell)
    draw_group("64" if cell.via == "find" else None if cell.via == "default" else cell.via)
    enc, o = _encode(cell)
    try:
        SEEN[cell.name] = _kernel_name(enc, cell.k)
        assert SEEN[cell.name] == batch_name(cell)
        if cell.name in UNLAUNCHABLE:
            _check_unlaunchable(enc, cell, S)
            return
        ref = oracle_reference(recipe_of(cell), S)
        check_instance_conditions(cell, ref)
        if cell.via == "find":
            draw_group(None)
            _check_find(enc, ref, cell.k, S)
            _check_status_panel(enc, ref, cell)
            return
        _check_sample(enc, ref, cell.k, S)
        if cell.family in ("solo8", "solo16", "lane", "wide"):
            _check_picks(enc, ref, cell.k, S)
        if cell.family in ("solo8", "solo16", "lane"):
            _check_fused_xt(enc, ref, cell.k, S)
        _check_status_panel(enc, ref, cell)
    finally:
        enc.close()


@pytest.mark.gpu
def test_every_cell_ran_its_kernel(gpu_available, request):
    """Every cell this session selected ran, and ran the instantiation it names (the per-cell assert
    guards the single case; this one guards the parametrisation)."""
    selected = {item.callspec.params["cell"].name for item in request.session.items
                if getattr(item, "originalname", "") == "test_cell_matches_oracle" and item.module is
                request.module}
    assert selected, "run together with the cells"
    assert set(SEEN) == selected
    assert {n: SEEN[n] for n in selected} == {n: batch_name(BY_NAME[n]) for n in selected}
    if len(selected) == len(CELLS):
        observed = {SEEN[c.name].replace("false>", "true>") if c.via == "find" else SEEN[c.name] for c in CELLS}
        assert observed == set(pkg("_native").draw_kernel_list())
