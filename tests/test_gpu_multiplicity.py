"""Panel multiplicities on the device: csa_unique_mult_async (uq_mult_kernel after the partitioning passes,
unique_mult_kernel + mult_emit_kernel on the single table), csa_mult_spectrum_async, and
analysis.legacy_panel_distribution.

The forged inputs of tests/distinct_cases.py go through both paths; the expected (first index,
multiplicity) pairs come from np.unique over the concatenated (h1, h2, row) triples, which knows nothing
of the code under test.  The product call is held to the reference's own panel counts
(tests/golden/multiplicity_<case>.json) and to the C oracle's panels through
stats.panel_multiplicities_host.  Every assertion is integer equality."""
import functools
import pickle
import random

import numpy as np
import pytest

import distinct_cases as C
from conftest import inst_paths, pkg
from oracle import coracle
from oracle.legacy_oracle import read_instance as oracle_read
from multiplicity_cases import CASES, expected_top, mult_golden, oracle_panels

pytestmark = pytest.mark.gpu

FORGED = ["threshold_65535", "threshold_65536", "threshold_65537", "collision_chains", "slot_pileup", "full_pileup",
          "one_partition_full", "skewed_large", "honest_large_1050001"]
MS_LDS_BINS = 8192      # kMsLdsBins: mult_spectrum_kernel's LDS histogram serves n_bins up to here
POISON = 0xFFFFFFFF


@functools.lru_cache(maxsize=2)
def _case(name):
    h, p, expected = C.UNIQUE_CASES[name]()
    return h, p, expected, _expected_pairs(h, p)


def _expected_pairs(h, p):
    """(first, mult) ascending in first: np.unique over the (h1, h2, row) triples."""
    _, first, mult = np.unique(np.concatenate([h, p], axis=1), axis=0, return_index=True, return_counts=True)
    order = np.argsort(first)
    return first[order].astype(np.int64), mult[order].astype(np.int64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel()).cuda()


def _mult(h, p, n=None):
    """csa_unique_mult_async over the first n entries of h / p (default: all) with fresh scratch, the
    lists poisoned and d_distinct preset to a wrong value.  Returns (first, mult) sorted by first (the
    list's own length), the length, and the status words."""
    import torch
    N = pkg("_native")
    L = N.lib()
    n = len(h) if n is None else n
    W = p.shape[1]
    dh, dp = _dev(h), _dev(p)
    need = int(L.csa_unique_mult_scratch_bytes(n))
    scratch = torch.full(((need + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    first = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    mult = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    distinct = torch.full((1,), 123456789, dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    N.check(L.csa_unique_mult_async(N.ptr(dh), N.ptr(dp), n, W, N.ptr(scratch), need, N.ptr(first), N.ptr(mult),
                                    N.ptr(distinct), N.ptr(status), None))
    torch.cuda.synchronize()
    ln = int(distinct.item())
    assert 0 <= ln <= n
    f = first.cpu().numpy().view(np.uint32)[:ln].astype(np.int64)
    m = mult.cpu().numpy().view(np.uint32)[:ln].astype(np.int64)
    assert (first.cpu().numpy()[ln:] == -1).all() and (mult.cpu().numpy()[ln:] == -1).all()   # nothing past the list
    order = np.argsort(f, kind="stable")
    return f[order], m[order], ln, status.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("name", FORGED)
def test_forged_cases_both_paths(gpu_available, monkeypatch, name):
    """The set of (first, multiplicity) pairs is np.unique's, the list is as long as the constructed
    distinct count, the multiplicities sum to n and the status block stays clean -- on the
    dispatcher's own path (the partitioned pass from 65 536 entries on) and on the single table."""
    h, p, expected, (want_f, want_m) = _case(name)
    n = len(h)
    assert len(want_f) == expected and int(want_m.sum()) == n
    assert C.takes_partitioned(n, C.table_slots(n)) == (n >= C.PART_MIN)
    for mode in (None, "0"):
        if mode is None:
            monkeypatch.delenv("CSA_UNIQUE_PART", raising=False)
        else:
            monkeypatch.setenv("CSA_UNIQUE_PART", mode)
        f, m, ln, st = _mult(h, p)
        print("%s CSA_UNIQUE_PART=%s: n %d expected %d list %d sum %d max %d status %s"
              % (name, mode, n, expected, ln, int(m.sum()), int(m.max()), st.tolist()))
        assert st[0] == 0
        assert ln == expected
        assert int(m.sum()) == n
        assert np.array_equal(f, want_f) and np.array_equal(m, want_m)


def test_one_partition_over(gpu_available, monkeypatch):
    """8193 distinct panels in one partition: the partitioned path leaves CSA_E_UNSUPPORTED in the status
    block (never a silently short list), the single table lists all 8193."""
    N = pkg("_native")
    h, p, expected, (want_f, want_m) = _case("one_partition_over")
    assert expected == C.K_UQ_TABLE + 1
    monkeypatch.delenv("CSA_UNIQUE_PART", raising=False)
    _, _, ln, st = _mult(h, p)
    print("one_partition_over partitioned: list %d status %s" % (ln, st.tolist()))
    assert st[0] == N.CSA_E_UNSUPPORTED
    with pytest.raises(N.CsaError, match="LDS table"):
        N.check(N.lib().csa_status_decode(N.ptr(st)))
    monkeypatch.setenv("CSA_UNIQUE_PART", "0")
    f, m, ln, st = _mult(h, p)
    assert st[0] == 0 and ln == expected
    assert np.array_equal(f, want_f) and np.array_equal(m, want_m)


def test_one_panel_70000_times(gpu_available, monkeypatch):
    """Every add on one LDS address: one entry, multiplicity 70 000, first index 0 (partitioned path)."""
    monkeypatch.delenv("CSA_UNIQUE_PART", raising=False)
    n = 70000
    row = np.array([[0x0123456789ABCDEF, 0x0F0F, 7]], np.uint64)
    p = np.repeat(row, n, axis=0)
    h = np.repeat(C.honest_hashes(row), n, axis=0)
    assert C.takes_partitioned(n, C.table_slots(n))
    f, m, ln, st = _mult(h, p)
    assert st[0] == 0 and ln == 1
    assert f.tolist() == [0] and m.tolist() == [n]


def test_no_panels_writes_zero(gpu_available):
    h, p = np.zeros((4, 2), np.uint64), np.zeros((4, 1), np.uint64)
    f, m, ln, st = _mult(h, p, n=0)
    assert ln == 0 and st[0] == 0 and len(f) == 0


def _spectrum(mult, length, n_bins):
    """csa_mult_spectrum_async over a device list of len(mult) entries (the capacity) of which `length`
    are valid; outputs poisoned beforehand."""
    import torch
    N = pkg("_native")
    d_mult = torch.from_numpy(np.asarray(mult, np.int64).astype(np.uint32).view(np.int32)).cuda()
    d_len = torch.full((1,), length, dtype=torch.int64, device="cuda")
    spectrum = torch.full((n_bins,), -7, dtype=torch.int64, device="cuda")
    summary = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    N.check(N.lib().csa_mult_spectrum_async(N.ptr(d_mult), N.ptr(d_len), len(mult), N.ptr(spectrum), n_bins,
                                            N.ptr(summary), None))
    torch.cuda.synchronize()
    return spectrum.cpu().numpy(), [int(x) for x in summary.cpu().numpy()]


@pytest.mark.parametrize("n_bins", [1, 7, 4096, MS_LDS_BINS, MS_LDS_BINS + 1])
def test_spectrum_against_numpy(gpu_available, n_bins):
    """A hand-made list longer than one pass of the grid (512 workgroups x 256), shorter than its
    capacity, the tail poisoned: bins, overflow, max, sum of squares and sum as numpy counts them."""
    rng = np.random.default_rng(11)
    length, capacity = 140007, 150001
    m = np.ones(capacity, np.int64)                              # half the list is singletons
    m[: length // 2] = rng.integers(1, 12, size=length // 2)
    m[1000:1400] = rng.integers(4000, 9000, size=400)            # around 4096 and the LDS form's end
    m[5] = 70000
    m[77] = 0                                                    # bin 0 is a bin like any other
    m[:length] = m[:length][rng.permutation(length)]
    m[length - 1] = MS_LDS_BINS                                  # the last valid entry, one past the LDS bins
    m[length:] = POISON
    valid = m[:length]
    spectrum, (over, top, sq, total) = _spectrum(m, length, n_bins)
    want = np.bincount(valid[valid < n_bins], minlength=n_bins)
    print("n_bins %d: overflow %d max %d sum m^2 %d sum m %d" % (n_bins, over, top, sq, total))
    assert np.array_equal(spectrum, want)
    assert over == int((valid >= n_bins).sum())
    assert top == int(valid.max()) == 70000
    assert sq == int((valid * valid).sum())
    assert total == int(valid.sum())


def test_spectrum_empty_list(gpu_available):
    spectrum, summary = _spectrum(np.full(300, POISON, np.int64), 0, 9)
    assert spectrum.tolist() == [0] * 9 and summary == [0, 0, 0, 0]


# ---- the product call ---------------------------------------------------------------------------
def _inst(name, k):
    cat, resp = inst_paths(name)
    return pkg().read_instance(cat, resp, k)


def _check_same_first_three(inst, S, seed, out, rng=None, keep_panels=True):
    alloc, found, hist = pkg("analysis").legacy_probabilities(inst, S, seed, rng=rng, keep_panels=keep_panels)
    assert out[0] == alloc
    assert len(out[1]) == len(found)
    if keep_panels:
        assert set(out[1]) == set(found)
    assert np.array_equal(out[2].upper(), hist.upper())


def _check_against_host(dist, panels, S, top=5):
    """A PanelDistribution against stats.panel_multiplicities_host of the same run's panels."""
    ST = pkg("stats")
    first, mult = ST.panel_multiplicities_host(panels)
    assert dist.S == S and dist.distinct == len(first)
    f, m = dist.multiplicities()
    assert np.array_equal(f, first) and np.array_equal(m, mult)
    assert dist.spectrum.tolist() == np.bincount(mult, minlength=1).tolist()
    assert dist.max_multiplicity == (int(mult.max()) if len(mult) else 0)
    assert dist.sum_squares == int((mult * mult).sum())
    n = dist._n
    host = ST.PanelDistribution(S, first, mult, panels, n, dist._ids)
    assert dist.top(top) == host.top(top)
    return first, mult


@pytest.mark.parametrize("case", CASES)
def test_panel_distribution_equals_the_reference(gpu_available, case):
    g = mult_golden(case)
    inst = _inst(g["instance"], g["k"])
    out = pkg("analysis").legacy_panel_distribution(inst, g["S"], g["seed"])
    assert len(out) == 4
    _check_same_first_three(inst, g["S"], g["seed"], out)
    dist = out[3]
    assert dist.S == g["S"] and dist.distinct == len(out[1]) == g["unique"]
    f, m = dist.multiplicities()
    assert f.tolist() == g["first"] and m.tolist() == g["count"]
    assert dist.spectrum.tolist() == np.bincount(np.array(g["count"])).tolist()
    assert dist.top(5) == expected_top(g, 5)
    assert dist.top(len(g["count"]) + 3) == expected_top(g, len(g["count"]))
    for e in (0, len(g["panels"]) // 2, len(g["panels"]) - 1):
        assert dist.count(g["panels"][e]) == g["count"][e]
    # the device-backed object pickles to host arrays
    back = pickle.loads(pickle.dumps(dist))
    assert isinstance(back._first, np.ndarray) and isinstance(back._panels, np.ndarray)
    assert back.top(5) == expected_top(g, 5) and back.count(g["panels"][0]) == g["count"][0]
    assert [a.tolist() for a in back.multiplicities()] == [g["first"], g["count"]]


def test_overflowing_spectrum_takes_the_second_pass(gpu_available):
    """pathological_5 at S = 20 000: three panels, the top one 6 788 times -- beyond the 4096 bins of
    the call's first pass."""
    A = pkg("analysis")
    S, seed = 20000, 0
    inst = _inst("pathological_5", 5)
    panels = oracle_panels("pathological_5", 5, seed, S)
    out = A.legacy_panel_distribution(inst, S, seed)
    _check_same_first_three(inst, S, seed, out)
    first, mult = _check_against_host(out[3], panels, S)
    assert len(first) == 3 and int(mult.max()) == 6788 > A.MULT_BINS
    assert out[3].max_multiplicity == 6788 and len(out[3].spectrum) == 6789


def test_mixed_shape_partitioned(gpu_available, monkeypatch, tmp_path):
    """30 agents (12 + 18 over one category, quotas 1..4 each), k = 5, S = 70 001, seed 5: 39 209 distinct
    panels with multiplicities 1..8, through the partitioned path."""
    monkeypatch.delenv("CSA_UNIQUE_PART", raising=False)
    cat, resp = tmp_path / "categories.csv", tmp_path / "respondents.csv"
    cat.write_text("category,feature,min,max\ngender,female,1,4\ngender,male,1,4\n")
    resp.write_text("gender\n" + "female\n" * 12 + "male\n" * 18)
    k, S, seed = 5, 70001, 5
    assert C.takes_partitioned(S, C.table_slots(S))
    rc, panels, _, _ = coracle.draw(oracle_read(str(cat), str(resp), k), k, seed, 0, S)
    assert rc == 0
    inst = pkg().read_instance(str(cat), str(resp), k)
    out = pkg("analysis").legacy_panel_distribution(inst, S, seed)
    first, mult = _check_against_host(out[3], panels, S)
    assert len(out[1]) == len(first) == 39209
    assert out[3].spectrum.tolist() == [0, 19197, 12315, 5331, 1774, 485, 92, 12, 3]
    assert out[3].coverage() == 1 - 19197 / 70001
    assert out[3].chao1() == 39209 + 19197 * 19196 / (2 * 12316)


def test_all_singletons(gpu_available):
    S, seed = 20011, 0
    inst = _inst("sf_e_110", 110)
    out = pkg("analysis").legacy_panel_distribution(inst, S, seed)
    dist = out[3]
    _check_against_host(dist, oracle_panels("sf_e_110", 110, seed, S), S, top=2)
    assert dist.distinct == S == len(out[1]) and dist.spectrum.tolist() == [0, S]
    assert dist.coverage() == 0.0 and dist.collision_probability() == 0.0 and dist.max_probability() == 1 / S
    assert dist.multiplicities()[0].tolist() == list(range(S))


def test_mt_mode(gpu_available):
    A, LG = pkg("analysis"), pkg("legacy")
    name, k, S, seed = "couples_panel_from_twenty_people_no_constraints_2", 2, 2000, 3
    inst = _inst(name, k)
    out = A.legacy_panel_distribution(inst, S, seed, rng="mt")
    _check_same_first_three(inst, S, seed, out, rng="mt")
    random.seed(seed)
    _, panels, _ = LG.mt_draw(pkg().encode(inst.categories, inst.agents), k, S)
    _check_against_host(out[3], panels, S)


def test_two_chunks(gpu_available):
    name, k, S, seed = "couples_panel_from_twenty_people_no_constraints_2", 2, (1 << 20) + 1000, 1
    inst = _inst(name, k)
    out = pkg("analysis").legacy_panel_distribution(inst, S, seed)
    first, mult = _check_against_host(out[3], oracle_panels(name, k, seed, S), S)
    assert len(first) == len(out[1]) == 100 and int(mult.sum()) == S


def test_panels_not_kept(gpu_available):
    A = pkg("analysis")
    g = mult_golden("couples_s0")
    inst = _inst(g["instance"], g["k"])
    out = A.legacy_panel_distribution(inst, g["S"], g["seed"], keep_panels=False)
    _check_same_first_three(inst, g["S"], g["seed"], out, keep_panels=False)
    dist = out[3]
    assert dist.spectrum.tolist() == np.bincount(np.array(g["count"])).tolist()
    assert [a.tolist() for a in dist.multiplicities()] == [g["first"], g["count"]]
    assert dist.chao1() == g["unique"] + 0.0 and dist.coverage() == 1.0
    for call in (lambda: dist.top(1), lambda: dist.count(g["panels"][0])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == A.PanelSet._where


def test_no_iterations(gpu_available):
    inst = _inst("couples_panel_from_twenty_people_no_constraints_2", 2)
    dist = pkg("analysis").legacy_sample_device(pkg().encode(inst.categories, inst.agents), 2, 0, 0,
                                                multiplicity=True).multiplicity
    assert len(dist["first"]) == 0 and dist["spectrum"].tolist() == [0] and dist["sum_squares"] == 0
