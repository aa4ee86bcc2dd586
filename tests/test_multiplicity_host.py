"""Panel multiplicities, host side: ``stats.panel_multiplicities_host`` over the C oracle's panels against
the reference's own panel counts (tests/golden/multiplicity_<case>.json, tools/make_multiplicity_goldens.py),
``stats.PanelDistribution`` (spectrum, estimators against values written out by hand, top with a forced tie,
degenerate runs, pickling into a process without a GPU), and the argument checks of the two C entry points
that return before any device call.  No GPU."""
import ctypes
import itertools
import json
import os
import pickle
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import distinct_cases as C
from conftest import REPO, inst_paths, pkg
from multiplicity_cases import CASES, expected_top, mult_golden, oracle_panels, pack


@pytest.fixture(scope="module", params=CASES)
def case(request):
    g = mult_golden(request.param)
    return g, oracle_panels(g["instance"], g["k"], g["seed"], g["S"])


def test_goldens_describe_the_philox_goldens():
    from conftest import golden
    for name in CASES:
        g, ph = mult_golden(name), golden(name)
        assert g["panels_sha256"] == ph["panels_sha256"] and g["unique"] == ph["unique"] == len(g["panels"])
        assert sum(g["count"]) == g["S"] == ph["S"]
        assert g["first"] == sorted(g["first"]) and len(set(g["first"])) == len(g["first"])


def test_host_multiplicities_equal_the_reference(case):
    g, panels = case
    first, mult = pkg("stats").panel_multiplicities_host(panels)
    assert first.dtype == np.int64 and mult.dtype == np.int64
    assert first.tolist() == g["first"]
    assert mult.tolist() == g["count"]
    assert np.array_equal(panels[first], pack(g["panels"], g["n"]))


def test_panel_distribution_from_the_goldens(case):
    g, panels = case
    S = pkg("stats")
    first, mult = S.panel_multiplicities_host(panels)
    ids = list(range(g["n"]))
    # handed over in another order: the class sorts by first index itself
    flip = np.arange(len(first))[::-1]
    d = S.PanelDistribution(g["S"], first[flip], mult[flip], panels, g["n"], ids)
    assert d.S == g["S"] and d.distinct == len(d) == g["unique"]
    spectrum = np.bincount(np.array(g["count"]))
    assert d.spectrum.dtype == np.int64 and d.spectrum.tolist() == spectrum.tolist()
    assert d.max_multiplicity == max(g["count"]) == len(d.spectrum) - 1
    assert d.sum_squares == sum(c * c for c in g["count"])
    f, m = d.multiplicities()
    assert f.tolist() == g["first"] and m.tolist() == g["count"]
    assert d.top(5) == expected_top(g, 5)
    assert d.top(10 ** 6) == expected_top(g, len(g["count"]))
    for e in (0, len(g["panels"]) - 1):
        assert d.count(g["panels"][e]) == g["count"][e]
        assert d.count(list(reversed(g["panels"][e]))) == g["count"][e]
    absent = next(p for p in itertools.combinations(range(g["n"]), g["k"]) if list(p) not in g["panels"])
    assert d.count(absent) == 0
    assert d.coverage() == 1 - int(spectrum[1]) / g["S"]
    assert d.max_probability() == max(g["count"]) / g["S"]


def _dist(mult, **kw):
    """A PanelDistribution over hand-made multiplicities, panel e = {e} (one word), first draws in order."""
    S = pkg("stats")
    mult = np.asarray(mult, np.int64)
    total = int(mult.sum())
    first = np.arange(len(mult), dtype=np.int64)
    # draws: every panel once in order, then the remaining copies
    seq = np.concatenate([first, np.repeat(first, mult - 1)]) if len(mult) else first
    panels = (np.uint64(1) << seq.astype(np.uint64)).reshape(-1, 1)
    return S.PanelDistribution(total, first, mult, panels, 64, list(range(64)), **kw)


def test_estimators_by_hand():
    # all singletons: 5 draws, 5 panels
    d = _dist([1, 1, 1, 1, 1])
    assert d.spectrum.tolist() == [0, 5] and d.max_multiplicity == 1
    assert d.coverage() == 0.0                       # 1 - 5/5
    assert d.chao1() == 15.0                         # 5 + 5*4 / (2*(0+1))
    assert d.collision_probability() == 0.0          # (5 - 5) / (5*4)
    assert d.max_probability() == 0.2
    # one panel 7 times
    d = _dist([7])
    assert d.spectrum.tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert d.coverage() == 1.0                       # f1 = 0
    assert d.chao1() == 1.0                          # D + 0
    assert d.collision_probability() == 1.0          # (49 - 7) / (7*6)
    assert d.max_probability() == 1.0
    # a mix: S = 12, D = 6, f1 = 3, f2 = 2, f5 = 1, sum m^2 = 3 + 8 + 25 = 36
    d = _dist([1, 2, 1, 5, 2, 1])
    assert d.S == 12 and d.distinct == 6 and d.spectrum.tolist() == [0, 3, 2, 0, 0, 1]
    assert d.sum_squares == 36
    assert d.coverage() == 0.75                      # 1 - 3/12
    assert d.chao1() == 7.0                          # 6 + 3*2 / (2*(2+1))
    assert d.collision_probability() == 24 / 132     # (36 - 12) / (12*11)
    assert d.max_probability() == 5 / 12


def test_degenerate_runs():
    d = _dist([])                                    # S = 0
    assert d.S == 0 and d.distinct == 0 and d.spectrum.tolist() == [0] and d.max_multiplicity == 0
    assert (d.coverage(), d.chao1(), d.collision_probability(), d.max_probability()) == (0.0, 0.0, 0.0, 0.0)
    assert d.top(3) == [] and d.count([1]) == 0
    assert [a.tolist() for a in d.multiplicities()] == [[], []]
    d = _dist([1])                                   # S = 1
    assert d.spectrum.tolist() == [0, 1]
    assert (d.coverage(), d.chao1(), d.collision_probability(), d.max_probability()) == (0.0, 1.0, 0.0, 1.0)
    d = _dist([2, 3])                                # f1 = 0
    assert d.coverage() == 1.0 and d.chao1() == 2.0
    with pytest.raises(ValueError):                  # multiplicities that do not sum to S
        pkg("stats").PanelDistribution(4, [0, 1], [2, 3])


def test_top_breaks_ties_by_first_index():
    d = _dist([2, 4, 1, 4, 2, 4])
    assert d.top(3) == [((1,), 4), ((3,), 4), ((5,), 4)]
    assert d.top(5) == [((1,), 4), ((3,), 4), ((5,), 4), ((0,), 2), ((4,), 2)]
    assert d.top(0) == []
    assert d.count((3,)) == 4 and d.count((2,)) == 1 and d.count((9,)) == 0
    with pytest.raises(KeyError):
        d.count((64,))


def test_without_panels_the_estimators_work_and_top_raises():
    S, A = pkg("stats"), pkg("analysis")
    d = S.PanelDistribution(12, [0, 1, 2, 3, 4, 5], [1, 2, 1, 5, 2, 1])
    assert d.spectrum.tolist() == [0, 3, 2, 0, 0, 1] and d.chao1() == 7.0
    for call in (lambda: d.top(1), lambda: d.count((0,))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == A.PanelSet._where
    back = pickle.loads(pickle.dumps(d))
    assert back.spectrum.tolist() == d.spectrum.tolist() and back.chao1() == 7.0
    with pytest.raises(RuntimeError):
        back.top(1)


_LOAD_CHILD = r"""
import json, pickle, sys
sys.path.insert(0, %(repo)r)
with open(%(path)r, "rb") as fh:
    d = pickle.load(fh)
assert "torch" not in sys.modules, "unpickling needed torch"
f, m = d.multiplicities()
print(json.dumps({"S": d.S, "distinct": d.distinct, "spectrum": d.spectrum.tolist(), "first": f.tolist(),
                  "mult": m.tolist(), "top": [[list(p), c] for p, c in d.top(4)], "count": d.count(%(panel)r),
                  "chao1": d.chao1(), "coverage": d.coverage(), "collision": d.collision_probability(),
                  "max": d.max_multiplicity}))
"""


def test_pickle_loads_in_a_child_without_gpu(tmp_path):
    g = mult_golden("couples_s0")
    panels = oracle_panels(g["instance"], g["k"], g["seed"], g["S"])
    S = pkg("stats")
    first, mult = S.panel_multiplicities_host(panels)
    d = S.PanelDistribution(g["S"], first, mult, panels, g["n"], list(range(g["n"])))
    path = tmp_path / "dist.pickle"
    with open(path, "wb") as fh:
        pickle.dump(d, fh)
    assert os.path.getsize(path) < 16 * 1024          # the distinct rows, not the S drawn ones
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = _LOAD_CHILD % dict(repo=REPO, path=str(path), panel=g["panels"][7])
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    assert got["S"] == g["S"] and got["distinct"] == g["unique"] and got["max"] == max(g["count"])
    assert got["first"] == g["first"] and got["mult"] == g["count"]
    assert got["spectrum"] == d.spectrum.tolist() == np.bincount(np.array(g["count"])).tolist()
    assert [(tuple(p), c) for p, c in got["top"]] == expected_top(g, 4)
    assert got["count"] == g["count"][7]
    assert (got["chao1"], got["coverage"], got["collision"]) == (d.chao1(), d.coverage(), d.collision_probability())


def test_counter_agrees_with_numpy_on_the_oracle_panels(case):
    """The host mirror against a plain Counter over the oracle's rows (no np.unique)."""
    g, panels = case
    seen = Counter(r.tobytes() for r in panels)
    first, mult = pkg("stats").panel_multiplicities_host(panels)
    assert [seen[panels[i].tobytes()] for i in first.tolist()] == mult.tolist() and len(seen) == len(first)


# ---- C ABI: what returns before any device call ---------------------------------------------------
def test_scratch_bytes_monotone_and_cover_the_partitioned_layout():
    L = pkg("_native").lib()
    ns = sorted({0, 1, 2, 31, 32, 33, 64, 1000, 4096, 4097, 65535, 65536, 65537, 70001, 1 << 20, (1 << 20) + 1,
                 1050001, 1 << 22, (1 << 22) + 1, 4200001, (1 << 23) + 5, 1 << 24, (1 << 24) + 1, 10 ** 8, (1 << 32) - 1})
    got = [int(L.csa_unique_mult_scratch_bytes(n)) for n in ns]
    assert got == sorted(got)
    for n, b in zip(ns, got):
        if n and C.fits(n):
            assert b >= C.scratch_bytes(n), n
        assert b >= 12 * C.table_slots(n), n           # the global table and its u32 counters


def test_invalid_arguments_return_before_any_device_call():
    N = pkg("_native")
    L = N.lib()
    word = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(word, ctypes.c_void_p)
    big = int(L.csa_unique_mult_scratch_bytes(5))
    bad = N.CSA_E_INVALID
    assert L.csa_unique_mult_async(p, p, 5, 0, p, big, p, p, p, p, None) == bad         # W < 1
    assert L.csa_unique_mult_async(p, p, 5, -3, p, big, p, p, p, p, None) == bad
    assert L.csa_unique_mult_async(None, p, 5, 1, p, big, p, p, p, p, None) == bad      # NULL with work to do
    assert L.csa_unique_mult_async(p, None, 5, 1, p, big, p, p, p, p, None) == bad
    assert L.csa_unique_mult_async(p, p, 5, 1, None, big, p, p, p, p, None) == bad
    assert L.csa_unique_mult_async(p, p, 5, 1, p, big, None, p, p, p, None) == bad
    assert L.csa_unique_mult_async(p, p, 5, 1, p, big, p, None, p, p, None) == bad
    assert L.csa_unique_mult_async(p, p, 5, 1, p, big, p, p, None, p, None) == bad
    assert L.csa_unique_mult_async(None, None, 0, 1, None, 0, None, None, None, None, None) == bad   # d_distinct
    assert L.csa_unique_mult_async(p, p, 5, 1, p, big - 1, p, p, p, p, None) == bad     # scratch too small
    assert "scratch" in N.last_error()
    assert L.csa_unique_mult_async(p, p, 1 << 32, 1, p, 1 << 62, p, p, p, p, None) == N.CSA_E_UNSUPPORTED
    assert L.csa_mult_spectrum_async(p, p, 5, p, 0, p, None) == bad                      # n_bins < 1
    assert L.csa_mult_spectrum_async(None, p, 5, p, 8, p, None) == bad
    assert L.csa_mult_spectrum_async(p, None, 5, p, 8, p, None) == bad
    assert L.csa_mult_spectrum_async(p, p, 5, None, 8, p, None) == bad
    assert L.csa_mult_spectrum_async(p, p, 5, p, 8, None, None) == bad


def test_sharded_runs_are_refused(monkeypatch):
    A, D = pkg("analysis"), pkg("distributed")
    cat, resp = inst_paths("couples_panel_from_twenty_people_no_constraints_2")
    inst = pkg().read_instance(cat, resp, 2)
    monkeypatch.setattr(D, "world_size", lambda: 2)
    for rng in (None, "mt"):
        with pytest.raises(NotImplementedError):
            A.legacy_panel_distribution(inst, 100, 0, rng=rng)
