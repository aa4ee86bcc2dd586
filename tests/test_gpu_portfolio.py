"""portfolio_pairs_kernel and the LEXIMIN / XMIN analysis entry points on the device
(analysis.py:194-228), bit for bit.

  * every tests/golden/portfolio_*.json (the unmodified reference's leximin_probabilities /
    xmin_probabilities on an injected portfolio) through ours with an injected find_distribution;
  * the kernel against the host ``add_portfolio_of_panels_to_histogram`` (pinned to the reference
    by tests/test_portfolio_host.py) on dense synthetic portfolios at the tile, n_pad, plane and
    staging-chunk edges.  The inputs are order-sensitive by construction: the test asserts on the
    host that the reversed sum differs in >= 5 % of the pairs wherever P >= 64, so a kernel that
    adds in another order cannot pass;
  * one long portfolio (many staging chunks), accumulation, the device-side sort, and the pickle
    loading where no GPU is visible.
"""
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, inst_paths, pkg
from test_portfolio_host import CASES, host_alloc, load

pytestmark = pytest.mark.gpu

CHUNK = 1024                       # panels staged per barrier pair (kPfPlanes * 32, csrc/portfolio.inc)
NS = [1, 2, 63, 64, 65, 257]
PS = [0, 1, 31, 32, 33, 63, 64, 65, 129, CHUNK - 1, CHUNK, CHUNK + 1]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def synthetic(n, P, seed, density=0.3):
    """P panels over n agents (position lists) at the given density, with duplicate panels, and
    weights over 12 binades with an exact 0.0 and a subnormal."""
    rs = np.random.RandomState(seed)
    x = rs.rand(P, n) < density
    for dst, src in ((3, 0), (40, 7), (P - 1, P // 2)):
        if 0 <= src < dst < P:
            x[dst] = x[src]
    w = rs.uniform(size=P) * 2.0 ** -rs.randint(0, 13, size=P).astype(np.float64)
    if P > 1:
        w[1] = 0.0
    if P > 2:
        w[2] = 3e-310
    return [np.flatnonzero(r).tolist() for r in x], [float(v) for v in w]


def host_prefixes(n, panels, weights, stops):
    """Host method over the first P panels for every P in ``stops``: {P: (triangle, alloc)}."""
    A = pkg("analysis")
    h, out, done = A.PairHistogram(n), {}, 0
    h._u = np.zeros(len(h), np.float64)
    for P in sorted(stops):
        h.add_portfolio_of_panels_to_histogram(panels[done:P], weights[done:P])
        done = P
        out[P] = (np.array(h.upper()), np.array(host_alloc(n, panels[:P], weights[:P]), np.float64))
    return out


def host_reversed(n, panels, weights):
    h = pkg("analysis").PairHistogram(n)
    h._u = np.zeros(len(h), np.float64)
    h.add_portfolio_of_panels_to_histogram(panels[::-1], weights[::-1])
    return np.array(h.upper())


def assert_order_sensitive(n, fwd, panels, weights):
    """A condition on the INPUTS: the same sum in reversed order has other bits in >= 5 % of pairs."""
    rev = host_reversed(n, panels, weights)
    differ = int(np.count_nonzero(bits(fwd) != bits(rev)))
    assert differ >= 0.05 * len(fwd), "inputs are not order-sensitive: %d of %d pairs differ" % (differ, len(fwd))


def device(n, panels, weights, upper0=None, alloc0=None, accumulate=False, want=(True, True)):
    """The transpose + kernel on position-list panels; outputs start as NaN unless given."""
    import torch
    A = pkg("analysis")
    m = n * (n - 1) // 2
    tri = alloc = None
    if want[0]:
        tri = torch.full((max(m, 1),), float("nan"), dtype=torch.float64, device="cuda")
        if upper0 is not None:
            tri[:m] = torch.from_numpy(np.ascontiguousarray(upper0)).cuda()
    if want[1]:
        alloc = torch.full((max(n, 1),), float("nan"), dtype=torch.float64, device="cuda")
        if alloc0 is not None:
            alloc[:n] = torch.from_numpy(np.ascontiguousarray(alloc0)).cuda()
    A._portfolio_launch(A._pack_positions(panels, n), np.array(weights, np.float64), n, tri, alloc,
                        accumulate=accumulate)
    torch.cuda.synchronize()
    return (tri[:m].cpu().numpy() if want[0] else None), (alloc[:n].cpu().numpy() if want[1] else None)


_MASTER = {}


def master(n):
    """One synthetic portfolio per n and the host results of its prefixes, computed once."""
    if n not in _MASTER:
        # n = 2 has one pair: its seed is one at which that pair's reversed sum differs at every P >= 64
        panels, weights = synthetic(n, max(PS), seed=201 if n == 2 else 100 + n)
        _MASTER[n] = (panels, weights, host_prefixes(n, panels, weights, PS))
    return _MASTER[n]


@pytest.mark.parametrize("n", NS)
def test_kernel_equals_host_method_bitwise(gpu_available, n):
    panels, weights, ref = master(n)
    for P in PS:
        tri, alloc = device(n, panels[:P], weights[:P])
        want_tri, want_alloc = ref[P]
        if P >= 64:
            assert_order_sensitive(n, want_tri, panels[:P], weights[:P])
        assert np.array_equal(bits(tri), bits(want_tri)), (n, P)
        assert np.array_equal(bits(alloc), bits(want_alloc)), (n, P)


def test_long_portfolio_many_chunks(gpu_available):
    n, P = 65, 20011
    panels, weights = synthetic(n, P, seed=9)
    ref = host_prefixes(n, panels, weights, [P])[P]
    assert_order_sensitive(n, ref[0], panels, weights)
    tri, alloc = device(n, panels, weights)
    assert np.array_equal(bits(tri), bits(ref[0]))
    assert np.array_equal(bits(alloc), bits(ref[1]))


def test_outputs_are_independent(gpu_available):
    """Either output alone gives the same values as both together."""
    n, P = 65, 129
    panels, weights, ref = master(n)
    tri, _ = device(n, panels[:P], weights[:P], want=(True, False))
    _, alloc = device(n, panels[:P], weights[:P], want=(False, True))
    assert np.array_equal(bits(tri), bits(ref[P][0])) and np.array_equal(bits(alloc), bits(ref[P][1]))


def test_accumulate_two_halves_equal_one_call(gpu_available):
    n, P, cut = 65, CHUNK + 1, 70
    panels, weights, ref = master(n)
    t1, a1 = device(n, panels[:cut], weights[:cut])
    t2, a2 = device(n, panels[cut:P], weights[cut:P], upper0=t1, alloc0=a1, accumulate=True)
    assert np.array_equal(bits(t2), bits(ref[P][0])) and np.array_equal(bits(a2), bits(ref[P][1]))
    # accumulating nothing keeps the stored values (a stored -0.0 included)
    t1[0] = -0.0
    t3, a3 = device(n, [], [], upper0=t1, alloc0=a1, accumulate=True)
    assert np.array_equal(bits(t3), bits(t1)) and np.array_equal(bits(a3), bits(a1))


def test_device_add_onto_prefilled_histogram(gpu_available):
    A = pkg("analysis")
    n, cut, P = 65, 33, 129
    panels, weights, _ = master(n)
    host, dev = A.PairHistogram(n), A.PairHistogram(n)
    for h in (host, dev):
        h.add_portfolio_of_panels_to_histogram(panels[:cut], weights[:cut])
    host.add_portfolio_of_panels_to_histogram(panels[cut:P], weights[cut:P])
    dev.add_portfolio_of_panels_to_histogram(panels[cut:P], weights[cut:P], device=True)
    assert dev._dtri is not None and dev._uv is None          # stays on the device until read
    dev.add_portfolio_of_panels_to_histogram(panels[P:P + 40], weights[P:P + 40], device=True)
    host.add_portfolio_of_panels_to_histogram(panels[P:P + 40], weights[P:P + 40])
    assert np.array_equal(bits(dev.upper()), bits(host.upper()))
    assert dev[(3, 1)] == host[(1, 3)]
    # integer weights keep the host path and stay ints
    ints = A.PairHistogram(n)
    ints.add_portfolio_of_panels_to_histogram(panels[:5], [1] * 5, device=True)
    assert ints._dtri is None and ints.upper().dtype.kind == "i"
    with pytest.raises(KeyError):
        A.PairHistogram(n).add_portfolio_of_panels_to_histogram([[0, n]], [0.5], device=True)


# ---- the public entry points against the reference's outputs -------------------------------------

def _instance(g):
    return pkg("analysis").read_instance(*inst_paths(g["instance"]), g["k"])


def _injected(g, inst, calls):
    ids = list(inst.agents)
    portfolio = [frozenset(ids[p] for p in panel) for panel in g["portfolio"]]

    def find_distribution(*args):
        calls.append(args)
        return portfolio, list(g["weights"]), []
    return portfolio, find_distribution


@pytest.mark.parametrize("case", CASES)
def test_goldens_through_public_entry_points(gpu_available, case):
    A = pkg("analysis")
    g = load(case)
    inst = _instance(g)
    n, ids = g["n"], list(inst.agents)
    for fn, key, threshold in ((A.leximin_probabilities, "leximin", 1e-11), (A.xmin_probabilities, "xmin", None)):
        calls = []
        portfolio, find = _injected(g, inst, calls)
        alloc, panels, hist = fn(inst, find_distribution=find)
        (cats, agents, columns, k, check, cols), = calls
        assert cats is inst.categories and agents is inst.agents and columns == {a: {} for a in ids}
        assert k == g["k"] and check is False and cols == []
        assert list(alloc) == ids
        assert np.array_equal(bits([alloc[a] for a in ids]), bits(g["alloc"]))
        assert isinstance(hist, A.PairHistogram) and hist._dtri is not None
        tri = np.ascontiguousarray(hist.upper(), "<f8")
        assert len(tri) == n * (n - 1) // 2
        assert hashlib.sha256(tri.tobytes()).hexdigest() == g["pairs_sha256"]
        if "pairs" in g:
            assert np.array_equal(bits(tri), bits(g["pairs"]))
        want = {p for p, w in zip(portfolio, g["weights"]) if threshold is None or w > threshold}
        assert isinstance(panels, set) and {frozenset(t) for t in panels} == want
        assert len(panels) == g[key + "_distinct"]
        pos = {a: q for q, a in enumerate(ids)}
        assert all(isinstance(t, tuple) and [pos[a] for a in t] == sorted(pos[a] for a in t) for t in panels)


def test_portfolio_probabilities_zip_and_threshold(gpu_available):
    A = pkg("analysis")
    g = load("couples")
    inst = _instance(g)
    ids = list(inst.agents)
    portfolio = [[ids[p] for p in panel] for panel in g["portfolio"]]
    # the shorter argument ends both, as zip in the reference
    alloc, panels, hist = A.portfolio_probabilities(inst, portfolio, g["weights"][:10])
    want = A.PairHistogram(g["n"])
    want.add_portfolio_of_panels_to_histogram(g["portfolio"][:10], g["weights"][:10])
    assert np.array_equal(bits(hist.upper()), bits(want.upper()))
    assert np.array_equal(bits([alloc[a] for a in ids]), bits(host_alloc(g["n"], g["portfolio"][:10], g["weights"][:10])))
    assert panels == {tuple(ids[p] for p in panel) for panel in g["portfolio"][:10]}
    # an empty portfolio: zeros everywhere
    alloc, panels, hist = A.portfolio_probabilities(inst, [], [])
    assert set(alloc.values()) == {0.0} and panels == set() and not hist.upper().any()
    _, panels, _ = A.portfolio_probabilities(inst, portfolio, g["weights"], min_probability=0.01)
    assert panels == {tuple(ids[p] for p in panel) for panel, w in zip(g["portfolio"], g["weights"]) if w > 0.01}


def test_sorted_pair_probabilities_sorts_on_the_device(gpu_available):
    A, St = pkg("analysis"), pkg("stats")
    g = load("example_small_20")
    inst = _instance(g)
    ids = list(inst.agents)
    _, _, hist = A.portfolio_probabilities(inst, [[ids[p] for p in panel] for panel in g["portfolio"]], g["weights"])
    got = St.sorted_pair_probabilities(hist)
    assert hist._dtri is not None and hist._uv is None        # sorted where it lies, not copied first
    assert got.dtype == np.float64 and np.array_equal(got, np.sort(hist.upper()))
    assert np.array_equal(St.sorted_pair_probabilities(hist), got)      # and on the host once it is read


_LOAD_CHILD = r"""
import pickle, sys
import numpy as np
sys.path.insert(0, %(repo)r)
with open(%(path)r, "rb") as fh:
    alloc, panels, hist = pickle.load(fh)
assert "torch" not in sys.modules, "unpickling needed torch"
np.save(%(alloc)r, np.array(list(alloc.values())))
np.save(%(upper)r, hist.upper())
print(len(panels))
"""


def test_returned_tuple_pickles_without_gpu(gpu_available, tmp_path):
    A = pkg("analysis")
    g = load("example_small_20")
    inst = _instance(g)
    _, find = _injected(g, inst, [])
    alloc, panels, hist = A.xmin_probabilities(inst, find_distribution=find)
    path = tmp_path / "xmin.pickle"
    with open(path, "wb") as fh:
        pickle.dump((alloc, panels, hist), fh)
    files = {key: str(tmp_path / (key + ".npy")) for key in ("alloc", "upper")}
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _LOAD_CHILD % dict(repo=REPO, path=str(path), **files)], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip()) == len(panels) == g["xmin_distinct"]
    assert np.array_equal(bits(np.load(files["alloc"])), bits(g["alloc"]))
    assert np.array_equal(bits(np.load(files["upper"])), bits(g["pairs"]))
