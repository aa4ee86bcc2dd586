"""The LEXIMIN / XMIN analysis side without a device (analysis.py:194-228).

  * the host ``PairHistogram.add_portfolio_of_panels_to_histogram`` equals every
    tests/golden/portfolio_*.json (outputs of the unmodified reference's leximin_probabilities /
    xmin_probabilities with an injected portfolio, tools/make_portfolio_goldens.py) bit for bit: it
    is the yardstick tests/test_gpu_portfolio.py holds the kernel to;
  * the goldens' inputs really are order-sensitive (a reversed sum differs);
  * csa_portfolio_pairs_async refuses invalid arguments on the host, before any device call;
  * leximin_probabilities / xmin_probabilities without an importable solver raise ImportError
    that names the keyword.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, inst_paths, pkg

CASES = sorted(f[len("portfolio_"):-len(".json")] for f in os.listdir(GOLD)
               if f.startswith("portfolio_") and f.endswith(".json"))


def load(case):
    """The golden's JSON with the arrays of the .npz beside it as lists: ``portfolio`` (position lists),
    ``alloc`` and, for n <= 200, ``pairs``."""
    with open(os.path.join(GOLD, "portfolio_%s.json" % case)) as fh:
        g = json.load(fh)
    with np.load(os.path.join(GOLD, "portfolio_%s.npz" % case), allow_pickle=False) as z:
        g.update({key: z[key].tolist() for key in z.files})
    return g


def host_triangle(n, portfolio, weights):
    h = pkg("analysis").PairHistogram(n)
    h.add_portfolio_of_panels_to_histogram(portfolio, weights)
    return np.ascontiguousarray(h.upper(), "<f8")


def host_alloc(n, portfolio, weights):
    """selection_probs of analysis.py:204-207: per agent, the panels' probabilities added in order."""
    a = [0.] * n
    for panel, w in zip(portfolio, weights):
        for p in panel:
            a[p] += w
    return a


def test_three_goldens_present():
    assert CASES == ["couples", "example_small_20", "sf_e_110"]


@pytest.mark.parametrize("case", CASES)
def test_host_method_equals_reference_bitwise(case):
    g = load(case)
    n, P = g["n"], g["P"]
    assert len(g["portfolio"]) == len(g["weights"]) == P
    assert 0.0 in g["weights"] and 1e-13 in g["weights"]
    tri = host_triangle(n, g["portfolio"], g["weights"])
    assert tri.dtype == np.float64 and len(tri) == n * (n - 1) // 2
    assert hashlib.sha256(tri.tobytes()).hexdigest() == g["pairs_sha256"]
    if "pairs" in g:
        assert np.array_equal(tri.view(np.uint64), np.array(g["pairs"], "<f8").view(np.uint64))
    assert np.array_equal(np.array(host_alloc(n, g["portfolio"], g["weights"])).view(np.uint64),
                          np.array(g["alloc"]).view(np.uint64))
    # the set sizes follow from the portfolio: every panel (XMIN), those above 1e-11 (LEXIMIN)
    assert g["xmin_distinct"] == len({frozenset(p) for p in g["portfolio"]}) == g["distinct_panels"]
    assert g["leximin_distinct"] == len({frozenset(p) for p, w in zip(g["portfolio"], g["weights"]) if w > 1e-11})


@pytest.mark.parametrize("case", ["example_small_20", "sf_e_110"])
def test_goldens_are_order_sensitive(case):
    g = load(case)
    fwd = host_triangle(g["n"], g["portfolio"], g["weights"])
    rev = host_triangle(g["n"], g["portfolio"][::-1], g["weights"][::-1])
    assert np.count_nonzero(fwd.view(np.uint64) != rev.view(np.uint64)) > 1000


def test_entry_point_refuses_invalid_arguments_on_the_host():
    N = pkg("_native")
    L = N.lib()
    buf = np.zeros(8, np.float64)          # host memory: never touched, every call is refused first
    xt = np.zeros(8, np.uint64)
    p, x = N.ptr(buf), N.ptr(xt)
    bad = [
        (x, 1, -1, p, p, p, 0),                                   # n < 0
        (None, 1, 4, p, p, p, 0),                                 # no XT with panels
        (x, 1, 4, p, None, None, 0),                              # both outputs NULL
        (x, 1, 4, p, p, p, 2),                                    # unknown flag bit
        (x, 1, 4, p, p, p, N.CSA_PORTFOLIO_ACCUMULATE | 0x80),
        (None, 0, 4, None, None, None, 0),                        # both outputs NULL even with no panels
    ]
    for args in bad:
        rc = L.csa_portfolio_pairs_async(*args, None)
        assert rc == N.CSA_E_INVALID, args
        assert "portfolio pairs" in N.last_error() and "invalid" in N.last_error()
    assert N.CSA_PORTFOLIO_ACCUMULATE == 1
    # n = 0 has nothing to write: accepted without a device call
    assert L.csa_portfolio_pairs_async(None, 0, 0, None, p, p, 0, None) == N.CSA_OK
    # accumulating no panels is a no-op, also without a device
    assert L.csa_portfolio_pairs_async(None, 0, 4, None, p, p, N.CSA_PORTFOLIO_ACCUMULATE, None) == N.CSA_OK
    assert not buf.any()
    assert L.csa_version() == 1


@pytest.mark.parametrize("fn,module,symbol", [("leximin_probabilities", "leximin", "find_distribution_leximin"),
                                              ("xmin_probabilities", "xmin", "find_distribution_xmin")])
def test_no_solver_importable_raises_import_error(monkeypatch, fn, module, symbol):
    A = pkg("analysis")
    monkeypatch.setitem(sys.modules, module, None)       # `import leximin` / `import xmin` now fail
    inst = A.read_instance(*inst_paths("example_small_20"), 20)
    with pytest.raises(ImportError) as e:
        getattr(A, fn)(inst)
    assert "find_distribution" in str(e.value) and symbol in str(e.value)


def test_unknown_agent_raises_key_error_before_any_device_work():
    A = pkg("analysis")
    inst = A.read_instance(*inst_paths("example_small_20"), 20)
    ids = list(inst.agents)
    with pytest.raises(KeyError):
        A.portfolio_probabilities(inst, [frozenset(ids[:19] + ["nobody"])], [1.0])
