"""analysis.legacy_sample_device asked for the group composition AND the multiplicities in one call: the
host copy then carries [counts | distinct count | statistics | multiplicity record | group table | status],
a layout no other test runs.  Every field must equal, as exact integers, what the two single-flag calls
(groups alone, multiplicity alone; tests/test_gpu_composition.py and tests/test_gpu_multiplicity.py hold
those to the oracle) give for the same draws: one chunk, three chunks, host-drawn panels, no panels, and
the lane kernel's fused-XT form on sf_e_110."""
import functools
import random

import numpy as np
import pytest

from conftest import inst_paths, pkg

pytestmark = pytest.mark.gpu

COUPLES = ("couples_panel_from_twenty_people_no_constraints_2", 2)
S, SEED = 3000, 9


@functools.lru_cache(maxsize=None)
def _setup(name, k):
    inst = pkg().read_instance(*inst_paths(name), k)
    return pkg().encode(inst.categories, inst.agents), pkg("stats").feature_groups(inst)


def _lists(m):
    """Host (first, multiplicity) pairs of the device lists, ascending in first index (the lists come
    in any order; each first index occurs once)."""
    first = m["first"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    mult = m["mult"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    order = np.argsort(first)
    return first[order].tolist(), mult[order].tolist()


@functools.lru_cache(maxsize=None)
def _single_flag(name, k, n_panels, mt):
    """The reference: the two single-flag calls over the same draws, once per case."""
    A = pkg("analysis")
    enc, groups = _setup(name, k)
    kw = _host_draw(enc, k, n_panels) if mt else {}
    comp = A.legacy_sample_device(enc, k, n_panels, SEED, groups=groups, **kw)
    mult = A.legacy_sample_device(enc, k, n_panels, SEED, multiplicity=True, **kw)
    assert comp.multiplicity is None and mult.composition is None
    return comp, mult, _lists(mult.multiplicity)


def _host_draw(enc, k, n_panels):
    random.seed(SEED)
    stats = np.zeros(3, np.uint64)
    _, panels, _ = pkg("legacy").mt_draw(enc, k, n_panels, stats=stats)
    return {"host_panels": panels, "host_stats": dict(zip(pkg("analysis").STAT_KEYS, (int(x) for x in stats)))}


def _check_combined(name, k, n_panels, mt=False, **kw):
    A = pkg("analysis")
    enc, groups = _setup(name, k)
    comp, mult, lists = _single_flag(name, k, n_panels, mt)
    if mt:
        kw.update(_host_draw(enc, k, n_panels))
    both = A.legacy_sample_device(enc, k, n_panels, SEED, groups=groups, multiplicity=True, **kw)
    assert both.composition.dtype == np.int64 and both.composition.shape == (len(groups), k + 1)
    assert np.array_equal(both.composition, comp.composition)
    assert int(both.composition.sum()) == len(groups) * n_panels              # every panel in one bin per group
    m, want = both.multiplicity, mult.multiplicity
    assert m["spectrum"].dtype == np.int64 and m["spectrum"].tolist() == want["spectrum"].tolist()
    assert type(m["sum_squares"]) is int and m["sum_squares"] == want["sum_squares"]
    assert _lists(m) == lists and sum(lists[1]) == n_panels
    for ref in (comp, mult):
        assert np.array_equal(both.counts, ref.counts) and both.counts.dtype == np.int64
        assert both.unique == ref.unique == len(lists[0])
        assert both.stats == ref.stats
        assert np.array_equal(np.triu(both.pairs.cpu().numpy()), np.triu(ref.pairs.cpu().numpy()))   # stored: i <= j
    assert int(both.counts.sum()) == k * n_panels
    return both


@pytest.mark.parametrize("chunk", [S, 1024])
def test_groups_and_multiplicity_in_one_call(gpu_available, chunk):
    """One chunk (the draw on the pipeline stream) and three (1024 + 1024 + 952, the chunk loop)."""
    both = _check_combined(*COUPLES, S, chunk=chunk)
    assert both.stats["attempts"] >= S


def test_groups_and_multiplicity_host_drawn_panels(gpu_available):
    """MT mode's form: the panels come from the host, every pass runs on the pipeline stream and the
    statistics are the host draw's (no statistics field in the copy)."""
    both = _check_combined(*COUPLES, S, mt=True)
    assert both.stats == _host_draw(_setup(*COUPLES)[0], 2, S)["host_stats"]


def test_groups_and_multiplicity_no_panels(gpu_available):
    both = _check_combined(*COUPLES, 0)
    assert not both.composition.any() and both.unique == 0 and both.multiplicity["spectrum"].tolist() == [0]
    assert not both.counts.any() and not both.pairs.cpu().numpy().any() and both.stats["attempts"] == 0


def test_groups_and_multiplicity_lane_kernel(gpu_available):
    """sf_e_110: draw_lane_kernel, whose one-chunk draw writes XT itself (counts from the pair diagonal)."""
    _check_combined("sf_e_110", 110, S)
