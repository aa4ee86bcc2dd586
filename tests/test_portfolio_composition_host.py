"""Weighted group composition of a LEXIMIN / XMIN portfolio, host side.

There is no reference function for this quantity: the yardstick is ``stats.group_whist_host`` (the
summation-order contract of csa_group_whist_async in numpy), and tests/test_gpu_portfolio_composition.py
holds the kernels to it bit for bit.  Here the yardstick itself is pinned three ways -- against a naive
triple loop, against the integer table of ``group_hist_host`` for weights of exactly 1.0, and against the
reference-pinned marginals of the three portfolio goldens -- and the synthetic inputs both files use are
shown to be order-sensitive, so that a kernel adding in another order cannot pass.  Then the ABI's
host-side refusals, WeightedCompositionHistogram, composition_difference and the entry points' argument
checks.  No GPU."""
import ctypes
import pickle
import re
import sys

import numpy as np
import pytest

from conftest import inst_paths, pkg
from test_gpu_portfolio import synthetic
from test_portfolio_host import CASES, load

# the shapes tests/test_gpu_portfolio_composition.py runs (kept here so that the order-sensitivity
# condition below covers every one of them)
BLOCK, UNROLL, CHUNK = 4, 32, 1024  # kWhBlock, kWhUnroll, kWhChunk (csrc/portfolio_composition.inc)
NS = [1, 63, 64, 65, 257]
GS = [1, 63, 64, 65, 130]
PS = sorted({0, 1, 2, BLOCK - 1, BLOCK, BLOCK + 1, UNROLL - 1, UNROLL, UNROLL + 1, 63, 64, 65, 129, CHUNK - 1, CHUNK, CHUNK + 1})
LONG = (257, 130, 40000)            # n, G, P: many chunks
BEYOND = (65, 5, 129)               # n, G, P of the bins = 5000 and bins = 20000 cases
WIDE = (8192, 3, 130)               # n, G, P of the W = 128 case: groups of <= 399 members, bins = 400
PORTFOLIO_SEED = {}           # n -> seed, where the default misses the order-sensitivity condition
GROUP_SEED = {}               # (n, G) -> seed, likewise


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def pack(panels, n):
    return pkg("analysis")._pack_positions(panels, n)


_MASTER = {}


def master(n, P=max(PS), seed=None):
    """One synthetic portfolio per (n, P) as test_gpu_portfolio builds them (duplicates, an exact 0.0
    weight, a subnormal, weights over 12 binades): (packed rows uint64[P, W], weights float64[P])."""
    key = (n, P)
    if key not in _MASTER:
        panels, weights = synthetic(n, P, seed=PORTFOLIO_SEED.get(n, 100 + n) if seed is None else seed)
        _MASTER[key] = (pack(panels, n), np.array(weights, np.float64))
    return _MASTER[key]


def make_groups(n, G, seed=None, cap=None):
    """uint64[G, W] masks of mixed densities (50 %, 10 %, 2 % in turn); from G = 3 on, the last two are
    the empty and the full group.  ``cap``: at most that many members per group."""
    rs = np.random.RandomState(GROUP_SEED.get((n, G), 7000 + 31 * n + G) if seed is None else seed)
    member = np.zeros((G, n), np.bool_)
    for g in range(G):
        member[g] = rs.uniform(size=n) < (0.50, 0.10, 0.02)[g % 3]
    if G >= 3:
        member[G - 2] = False
        member[G - 1] = True
    if cap is not None:
        for g in range(G):
            on = np.flatnonzero(member[g])
            member[g, on[cap:]] = False
    return pkg("stats")._pack_members(member, (n + 63) // 64)


def naive(masks, panels, weights, bins):
    """The contract as a triple Python loop: panel, group, bit count."""
    G = len(masks)
    hist = [[0.0] * bins for _ in range(G)]
    for p in range(len(panels)):
        for g in range(G):
            c = sum(bin(int(x) & int(m)).count("1") for x, m in zip(panels[p], masks[g]))
            hist[g][c] += float(weights[p])
    return np.array(hist, np.float64).reshape(G, bins)


def test_host_equals_naive_triple_loop_bitwise():
    St = pkg("stats")
    n, P, G = 65, 65, 64
    rows, w = master(n)
    rows, w = rows[:P], w[:P]
    assert w[1] == 0.0 and 0.0 < w[2] < 2.3e-308 and np.array_equal(rows[3], rows[0])
    assert np.log2(w[w > 1e-300].max() / w[w > 1e-300].min()) > 8
    masks = make_groups(n, G)
    sizes = St._popcount_rows(masks)
    assert sizes[G - 2] == 0 and sizes[G - 1] == n and 0 < sizes[2] < sizes[0]
    got = St.group_whist_host(masks, rows, w, n + 1)
    assert got.dtype == np.float64 and got.shape == (G, n + 1)
    assert np.array_equal(bits(got), bits(naive(masks, rows, w, n + 1)))
    # out= accumulates onto what it holds, in place
    half = St.group_whist_host(masks, rows[:30], w[:30], n + 1)
    again = St.group_whist_host(masks, rows[30:], w[30:], n + 1, out=half)
    assert again is half and np.array_equal(bits(half), bits(got))
    assert St.group_whist_host(masks, rows[:0], w[:0], 3).tolist() == [[0.0] * 3] * G
    assert St.group_whist_host(masks[:0], rows, w, 3).shape == (0, 3)


def test_host_count_past_bins_raises():
    St, N = pkg("stats"), pkg("_native")
    rows, w = master(65)
    masks = make_groups(65, 5)
    top = int(St._group_counts(masks, rows[:65]).max())
    St.group_whist_host(masks, rows[:65], w[:65], top + 1)
    with pytest.raises(N.CsaError) as e:
        St.group_whist_host(masks, rows[:65], w[:65], top)
    assert e.value.code == N.CSA_E_INVALID


def _golden(case):
    St = pkg("stats")
    g = load(case)
    inst = pkg("analysis").read_instance(*inst_paths(g["instance"]), g["k"])
    return g, inst, St.feature_groups(inst), pack(g["portfolio"], g["n"])


@pytest.mark.parametrize("case", CASES)
def test_unit_weights_give_the_integer_table(case):
    """Sums of ones are exact: the table is group_hist_host's, whatever the order."""
    St = pkg("stats")
    g, inst, groups, rows = _golden(case)
    k = g["k"]
    got = St.group_whist_host(groups.masks, rows, np.ones(len(rows)), k + 1)
    want = St.group_hist_host(groups.masks, rows, k + 1)
    assert np.array_equal(got, want.astype(np.float64)) and got.sum() == len(groups) * len(rows)


@pytest.mark.parametrize("case", CASES)
def test_against_reference_pinned_marginals(case):
    """Per group, sum_c c * values[g][c] and the golden alloc summed over the group's members are sums of
    the same P * k-or-fewer non-negative terms w[p] in different orders: (terms + the k + 2 roundings of
    the products and the outer sum) * 2^-53 relative bounds their difference.  Every row sums to the
    portfolio's total the same way."""
    St = pkg("stats")
    g, inst, groups, rows = _golden(case)
    k, P, n = g["k"], g["P"], g["n"]
    w = np.array(g["weights"], np.float64)
    values = St.group_whist_host(groups.masks, rows, w, k + 1)
    comp = St.WeightedCompositionHistogram(groups.labels, values, St.portfolio_total(w), P, k)
    member = np.unpackbits(groups.masks.view(np.uint8).reshape(len(groups), -1), axis=1, bitorder="little")[:, :n]
    alloc = g["alloc"]
    u = 2.0 ** -53
    for gi in range(len(groups)):
        lhs = sum(c * float(values[gi, c]) for c in range(k + 1))
        rhs = sum(alloc[i] for i in np.flatnonzero(member[gi]).tolist())
        assert abs(lhs - rhs) <= (P * k + k + 2) * u * max(lhs, rhs), (case, gi, lhs, rhs)
        row = sum(values[gi].tolist())
        assert abs(row - comp.total) <= (P + k + 1) * u * comp.total, (case, gi, row, comp.total)
    assert np.allclose(comp.mean(), [sum(alloc[i] for i in np.flatnonzero(m).tolist()) / comp.total for m in member],
                       rtol=1e-9, atol=0)


def wide_case():
    """n = 8192 (W = 128): three groups of at most 399 members, so that 400 bins hold every count."""
    n, G, P = WIDE
    rows, w = master(n, P, seed=4242)
    return make_groups(n, G, cap=399), rows, w


def bad_count_case():
    """n = 257, 200 panels, 10 groups; group 7 is agents 0..bins-1 and panel 120 is exactly those agents:
    the one (panel, group) whose count reaches bins.  Returns masks, rows, w, bins, bad panel, bad group."""
    St = pkg("stats")
    n, G, P, bad_panel, bad_group = 257, 10, 200, 120, 7
    rows, w = master(n)
    rows, w = rows[:P].copy(), w[:P].copy()
    masks = make_groups(n, G)
    one = np.zeros((1, n), np.bool_)
    one[0, 0] = True
    masks &= ~St._pack_members(one, 5)                      # agent 0 is in the bad group alone
    bins = int(St._group_counts(masks, rows).max()) + 1
    both = np.zeros((1, n), np.bool_)
    both[0, :bins] = True
    masks[bad_group] = rows[bad_panel] = St._pack_members(both, 5)[0]
    w[bad_panel] = 0.3
    c = St._group_counts(masks, rows)
    over = np.argwhere(c >= bins)
    assert over.tolist() == [[bad_panel, bad_group]], over
    return masks, rows, w, bins, bad_panel, bad_group


def order_sensitive_inputs():
    """(name, masks, rows, weights, bins) of every synthetic input with P >= 64 that the two files run."""
    for n in NS:
        rows, w = master(n)
        for G in GS:
            masks = make_groups(n, G)
            for P in PS:
                if P >= 64:
                    yield "n%d G%d P%d" % (n, G, P), masks, rows[:P], w[:P], n + 1
    n, G, P = LONG
    rows, w = master(n, P, seed=9)
    yield "long", make_groups(n, G), rows, w, n + 1
    n, G, P = BEYOND
    yield "beyond", make_groups(n, G), master(n)[0][:P], master(n)[1][:P], 5000
    masks, rows, w = wide_case()
    yield "wide", masks, rows, w, 400
    masks, rows, w, bins, bad_panel, _ = bad_count_case()
    keep = np.arange(len(rows)) != bad_panel
    yield "bad count", masks, rows[keep], w[keep], bins


def test_inputs_are_order_sensitive():
    """A condition on the INPUTS: the same sums in reversed panel order have other bits in >= 10 % of the
    entries that receive >= 3 panels.  (The unit-weight inputs are exact in any order by design; they
    check the counting, not the order.)"""
    St = pkg("stats")
    seen = []
    for name, masks, rows, w, bins in order_sensitive_inputs():
        fwd = St.group_whist_host(masks, rows, w, bins)
        rev = St.group_whist_host(masks, rows[::-1], w[::-1], bins)
        many = St.group_hist_host(masks, rows, bins) >= 3
        differ = int(np.count_nonzero((bits(fwd) != bits(rev)) & many))
        seen.append((name, differ, int(many.sum())))
        assert many.sum() and differ >= 0.10 * many.sum(), \
            "inputs are not order-sensitive: %s, %d of %d entries differ" % (name, differ, many.sum())
    assert len(seen) == len(NS) * len(GS) * sum(P >= 64 for P in PS) + 4


def test_goldens_own_weights_are_order_sensitive():
    St = pkg("stats")
    g, inst, groups, rows = _golden("sf_e_110")
    w = np.array(g["weights"], np.float64)
    fwd = St.group_whist_host(groups.masks, rows, w, g["k"] + 1)
    rev = St.group_whist_host(groups.masks, rows[::-1], w[::-1], g["k"] + 1)
    assert np.count_nonzero(bits(fwd) != bits(rev)) >= 10


# ---- the C ABI --------------------------------------------------------------------------------------

C_TYPES = {"const uint64_t *": ctypes.c_void_p, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32,
           "uint32_t": ctypes.c_uint32, "const double *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "uint32_t *": ctypes.c_void_p, "void *": ctypes.c_void_p}


def _declared_args(text, res, name):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), text)
    assert m, "%s is not declared in include/csa_legacy.h" % name
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        args.append(C_TYPES[re.match(r"(.*?)\w+$", a).group(1).strip()])
    return args


def test_group_whist_symbols_declared_as_bound():
    N = pkg("_native")
    with open(N.HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    res, bound = N.SIGNATURES["csa_group_whist_async"]
    args = _declared_args(text, "int", "csa_group_whist_async")
    assert res is ctypes.c_int and bound == args and len(args) == 11
    res, bound = N.SIGNATURES["csa_group_whist_scratch_bytes"]
    assert res is ctypes.c_uint64 and bound == _declared_args(text, "uint64_t", "csa_group_whist_scratch_bytes")
    res, bound = N.SIGNATURES["csa_group_whist_scratch"]
    assert res is ctypes.c_int and bound == _declared_args(text, "int", "csa_group_whist_scratch")
    assert re.search(r"#define\s+CSA_GROUP_WHIST_ACCUMULATE\s+0x1u", text) and N.CSA_GROUP_WHIST_ACCUMULATE == 1
    for name in ("csa_group_whist_async", "csa_group_whist_scratch_bytes", "csa_group_whist_scratch"):
        assert hasattr(N.lib(), name)
    assert N.lib().csa_version() == 1


def test_group_whist_refusals_and_noops_on_the_host():
    """Every refusal and no-op happens before any device call: null pointers, no device."""
    N = pkg("_native")
    L = N.lib()
    ACC = N.CSA_GROUP_WHIST_ACCUMULATE
    call = L.csa_group_whist_async
    #         panels P  W  weights masks G  bins hist flags status stream
    assert call(None, 5, 0, None, None, 1, 3, None, 0, None, None) == N.CSA_E_INVALID        # W < 1
    assert "group whist" in N.last_error() and "invalid" in N.last_error()
    assert call(None, 5, 2, None, None, 1, 0, None, 0, None, None) == N.CSA_E_INVALID        # bins < 1
    assert call(None, 5, 2, None, None, -1, 3, None, 0, None, None) == N.CSA_E_INVALID       # n_groups < 0
    assert call(None, 5, 2, None, None, 1, 3, None, 2, None, None) == N.CSA_E_INVALID        # unknown flag bit
    assert call(None, 5, 2, None, None, 1, 3, None, ACC | 0x80, None, None) == N.CSA_E_INVALID
    assert call(None, 5, 2, None, None, 0, 3, None, 0, None, None) == N.CSA_OK               # no groups: no-op
    assert call(None, 5, 2, None, None, 0, 3, None, ACC, None, None) == N.CSA_OK
    assert call(None, 0, 2, None, None, 4, 3, None, ACC, None, None) == N.CSA_OK             # nothing to add
    assert call(None, 0, 2, None, None, 4, 3, None, 0, None, None) == N.CSA_E_INVALID        # a table to zero: NULL
    assert call(None, 5, 2, None, None, 4, 3, None, 0, None, None) == N.CSA_E_INVALID        # needed pointers NULL
    one = ctypes.c_uint64(0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)
    for missing in range(5):                                                                # each needed pointer
        ptrs = [p] * 5
        ptrs[missing] = None
        assert call(ptrs[0], 5, 2, ptrs[1], ptrs[2], 4, 3, ptrs[3], 0, ptrs[4], None) == N.CSA_E_INVALID, missing
    assert call(p, 5, 8193, p, p, 4, 3, p, 0, p, None) == N.CSA_E_UNSUPPORTED                # refused before launch
    assert "8192" in N.last_error()
    # the count scratch is lent beforehand; without a loan of csa_group_whist_scratch_bytes the call is refused
    assert L.csa_group_whist_scratch_bytes(5, 4) == 5 * 4 * 4 and L.csa_group_whist_scratch_bytes(0, 4) == 0
    assert L.csa_group_whist_scratch_bytes(8635, 377) == 8635 * 377 * 4
    assert L.csa_group_whist_scratch(None, 0) == N.CSA_OK
    assert call(p, 5, 2, p, p, 4, 3, p, 0, p, None) == N.CSA_E_INVALID and "scratch" in N.last_error()
    assert L.csa_group_whist_scratch(p, 79) == N.CSA_OK
    assert call(p, 5, 2, p, p, 4, 3, p, 0, p, None) == N.CSA_E_INVALID and "scratch" in N.last_error()
    assert L.csa_group_whist_scratch(None, 8) == N.CSA_E_INVALID
    assert L.csa_group_whist_scratch(None, 0) == N.CSA_OK
    assert one.value == 0


# ---- WeightedCompositionHistogram, composition_difference ------------------------------------------

def _hand_made():
    St = pkg("stats")
    values = np.array([[0.5, 0.0, 1.5, 0.0], [0.0, 0.0, 0.0, 2.0], [2.0, 0.0, 0.0, 0.0], [0.25, 0.75, 0.75, 0.25]])
    return St.WeightedCompositionHistogram(["a", "b", "c", "d"], values, 2.0, 7, 3), values


def test_weighted_composition_histogram_values_and_pickle():
    St = pkg("stats")
    h, values = _hand_made()
    assert len(h) == 4 and h.P == 7 and h.k == 3 and h.total == 2.0
    assert np.array_equal(h.probabilities(), values / 2.0)
    assert h.mean().tolist() == [1.5, 3.0, 0.0, 1.5]
    assert h.panel_share().tolist() == [0.5, 1.0, 0.0, 0.5]
    assert h.variance().tolist() == [0.75, 0.0, 0.0, 0.75]
    assert h.prob_absent().tolist() == [0.25, 0.0, 1.0, 0.125]
    lo, hi = h.support()
    assert lo.tolist() == [0, 3, 0, 0] and hi.tolist() == [2, 3, 0, 3]
    back = pickle.loads(pickle.dumps(h))
    assert isinstance(back, St.WeightedCompositionHistogram) and back.labels == h.labels
    assert (back.total, back.P, back.k) == (2.0, 7, 3)
    assert isinstance(back.values, np.ndarray) and np.array_equal(bits(back.values), bits(values))
    empty = St.WeightedCompositionHistogram(["a"], np.zeros((1, 4)), 0.0, 0, 3)
    assert [x.tolist() for x in empty.support()] == [[-1], [-1]]
    with pytest.raises(AssertionError):
        St.WeightedCompositionHistogram(["a"], np.zeros((1, 5)), 1.0, 1, 3)


def test_composition_difference():
    St = pkg("stats")
    h, _ = _hand_made()
    counts = np.array([[2, 0, 6, 0], [0, 8, 0, 0], [8, 0, 0, 0], [1, 3, 3, 1]], np.int64)
    legacy = St.CompositionHistogram(["a", "b", "c", "d"], counts, 8, 3)
    d = St.composition_difference(legacy, h)
    assert d["labels"] == ["a", "b", "c", "d"]
    assert d["total_variation"].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert d["mean"].tolist() == [0.0, -2.0, 0.0, 0.0]
    assert d["prob_absent"].tolist() == [0.0, 0.0, 0.0, 0.0]
    back = St.composition_difference(h, legacy)
    assert back["mean"].tolist() == [0.0, 2.0, 0.0, 0.0] and back["total_variation"].tolist() == [0.0, 1.0, 0.0, 0.0]
    other = St.WeightedCompositionHistogram(["a", "b", "c", "d"], counts[::-1] / 4.0, 2.0, 8, 3)
    d2 = St.composition_difference(h, other)
    assert d2["total_variation"].tolist() == [0.5, 1.0, 1.0, 0.5]
    assert d2["prob_absent"].tolist() == [0.125, -1.0, 1.0, -0.125]
    with pytest.raises(ValueError):
        St.composition_difference(h, St.CompositionHistogram(["a", "b", "c", "e"], counts, 8, 3))
    with pytest.raises(ValueError):
        St.composition_difference(h, St.CompositionHistogram(["a", "b", "c", "d"], np.zeros((4, 5), np.int64), 8, 4))
    with pytest.raises(ValueError):
        St.composition_difference(h, counts)


# ---- entry points -----------------------------------------------------------------------------------

def _small():
    A = pkg("analysis")
    return A.read_instance(*inst_paths("example_small_20"), 20)


@pytest.mark.parametrize("fn,module,symbol", [("leximin_composition", "leximin", "find_distribution_leximin"),
                                              ("xmin_composition", "xmin", "find_distribution_xmin")])
def test_no_solver_importable_raises_import_error(monkeypatch, fn, module, symbol):
    A, St = pkg("analysis"), pkg("stats")
    monkeypatch.setitem(sys.modules, module, None)       # `import leximin` / `import xmin` now fail
    inst = _small()
    with pytest.raises(ImportError) as e:
        getattr(A, fn)(inst, St.feature_groups(inst))
    assert "find_distribution" in str(e.value) and symbol in str(e.value)


def test_groups_argument_is_checked_before_any_device_work():
    A, St = pkg("analysis"), pkg("stats")
    inst = _small()
    ids = list(inst.agents)

    def never(*args):
        raise AssertionError("the solver must not run")
    calls = (lambda g: A.portfolio_composition(inst, [ids[:20]], [1.0], g),
             lambda g: A.leximin_composition(inst, g, find_distribution=never),
             lambda g: A.xmin_composition(inst, g, find_distribution=never))
    for call in calls:
        with pytest.raises(TypeError):
            call(St.feature_groups(inst).masks)
    other = St.GroupSet(["x"], np.zeros((1, 2), np.uint64))     # W = 2, the instance has W = 1
    for call in calls:
        with pytest.raises(ValueError):
            call(other)


def test_public_names_are_exported():
    P = pkg()
    for name in ("leximin_composition", "xmin_composition", "portfolio_composition", "WeightedCompositionHistogram",
                 "composition_difference", "group_whist_host", "portfolio_group_composition"):
        assert name in P.__all__ and hasattr(P, name)


def test_portfolio_group_composition_takes_the_host_path_without_a_gpu(monkeypatch):
    import torch
    St = pkg("stats")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # no GPU visible
    calls = []
    host = St.group_whist_host
    monkeypatch.setattr(St, "group_whist_host", lambda *a, **kw: calls.append(1) or host(*a, **kw))
    g, inst, groups, rows = _golden("example_small_20")
    w = np.array(g["weights"], np.float64)
    comp = St.portfolio_group_composition(groups, rows, w, g["k"])
    assert calls == [1]
    assert isinstance(comp, St.WeightedCompositionHistogram) and comp.labels == groups.labels
    assert comp.P == g["P"] and comp.k == g["k"] and comp.total == sum(g["weights"], 0.)
    assert np.array_equal(bits(comp.values), bits(host(groups.masks, rows, w, g["k"] + 1)))
    with pytest.raises(ValueError):
        St.portfolio_group_composition(groups, rows, w[:-1], g["k"])
