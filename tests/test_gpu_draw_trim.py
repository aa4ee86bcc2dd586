"""GPU parity of the register draw kernels where their step loop was trimmed, against the C oracle.

Three places where the lane / solo / wide kernels do less work than a literal restatement of
legacy.py and must still give the reference's picks, attempts and restart statistics bit for bit:

  * the k-th pick's delete_all_in_cat is skipped for a panel that meets every minimum (nothing reads
    the pool or the remaining counts after it), while an under-quota panel still cascades so that its
    restart is classified as the reference classifies it (SelectionError, legacy.py:55, or min-quota
    rejection, legacy.py:160-168);
  * the two-lane kernel's second lane keeps the pool mirrored (words reversed and bit-reversed) and
    maps its find back to an agent index;
  * the slack bit planes (max - selected) are kept only as far as the instance's largest slack needs.

Every test compares the picks in pick order, the attempts per panel and the selection_errors /
rejections / attempts statistics with the oracle.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import pkg
from oracle import coracle
from oracle.legacy_oracle import OracleInstance
from oracle.philox import legacy_randint, legacy_word

pytestmark = pytest.mark.gpu


@pytest.fixture
def draw_group():
    """Force a batch draw layout (CSA_DRAW_KERNEL = "solo" / "lane" / "wide")."""
    old = os.environ.get("CSA_DRAW_KERNEL")

    def set_layout(g):
        os.environ["CSA_DRAW_KERNEL"] = str(g)
    yield set_layout
    if old is None:
        os.environ.pop("CSA_DRAW_KERNEL", None)
    else:
        os.environ["CSA_DRAW_KERNEL"] = old


def _kernel_name(enc, k):
    N = pkg("_native")
    buf = np.zeros(64, np.uint8)
    N.check(N.lib().csa_draw_kernel_name(enc.handle, k, buf.ctypes.data_as(ctypes.c_char_p), 64))
    return bytes(buf).split(b"\0")[0].decode()


def _draw_picks(enc, k, S, seed, begin, max_attempts=100000):
    """csa_draw_picks_async: (picks int32[S, k] in pick order, attempts uint32[S])."""
    import torch
    N = pkg("_native")
    assert N.lib().csa_draw_picks_supported(enc.handle, k) == 1
    kp = int(N.lib().csa_picks_stride(k))
    picks = torch.empty(S * kp, dtype=torch.int16, device="cuda")
    att = torch.empty(S, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    N.check(N.lib().csa_draw_picks_async(enc.handle, k, seed, begin, S, max_attempts, N.ptr(picks), N.ptr(att),
                                         N.ptr(status), None))
    torch.cuda.synchronize()
    assert int(status[0].item()) == 0
    return (picks.cpu().numpy().view(np.uint16).astype(np.int32).reshape(S, kp)[:, :k],
            att.cpu().numpy().astype(np.uint32))


def _sample_panels(enc, k, S, seed, begin, max_attempts=100000):
    """csa_legacy_sample (the draw with the fused pack where the kernel has one): panels, attempts."""
    N = pkg("_native")
    panels = np.zeros((S, enc.W), np.uint64)
    attempts = np.zeros(S, np.uint32)
    N.check(N.lib().csa_legacy_sample(enc.handle, k, seed, begin, S, N.CSA_WANT_PANELS, max_attempts,
                                      N.ptr(panels), None, None, None, N.ptr(attempts)))
    return panels, attempts


def _redraw_panels(enc, k, S, seed, begin, max_attempts=100000):
    """csa_redraw_async: the same draw with the statistics not requested (panels only)."""
    import torch
    N = pkg("_native")
    panels = torch.zeros(S * enc.W, dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    N.check(N.lib().csa_redraw_async(enc.handle, k, seed, begin, S, max_attempts, N.ptr(panels), N.ptr(status), None))
    torch.cuda.synchronize()
    assert int(status[0].item()) == 0
    return panels.cpu().numpy().view(np.uint64).reshape(S, enc.W)


def _check_against_oracle(enc, o, k, S, seed, begin):
    """Picks in pick order, attempts and statistics of one draw vs the C oracle (computed once and
    returned: (opanels, oatt, opicks, rejects))."""
    A = pkg("analysis")
    rejects = np.zeros(S, np.uint32)
    rc, opanels, oatt, opicks = coracle.draw(o, k, seed, begin, S, max_attempts=100000, want_picks=True,
                                             rejects=rejects)
    assert rc == 0
    want_stats = {"attempts": int(oatt.sum()), "rejections": int(rejects.sum()),
                  "selection_errors": int(oatt.sum()) - S - int(rejects.sum())}
    A.draw_stats(enc, reset=True)
    picks, att = _draw_picks(enc, k, S, seed, begin)
    stats = A.draw_stats(enc)
    assert np.array_equal(att, oatt)
    assert np.array_equal(picks, opicks)
    assert stats == want_stats
    # the same draw through the fused pack (chunked pick lists) where the kernel has one
    A.draw_stats(enc, reset=True)
    panels, att2 = _sample_panels(enc, k, S, seed, begin)
    stats2 = A.draw_stats(enc)
    assert np.array_equal(att2, oatt)
    assert np.array_equal(panels, opanels)
    assert stats2 == want_stats
    return opanels, oatt, opicks, rejects


def _pool(F_per_cat, n, k, seed, lo, hi):
    """Random pool: categories with the given feature counts, shares ~ Dirichlet(2), quotas
    floor(lo k p) / ceil(hi k p).  Returns (categories, fmin, fmax, fcat, person_feat)."""
    rng = np.random.default_rng(seed)
    cats, fmin, fmax, fcat, cols, base = {}, [], [], [], [], 0
    for c, nf in enumerate(F_per_cat):
        p = rng.dirichlet(np.full(nf, 2.0))
        cats["c%d" % c] = {}
        for j in range(nf):
            a, b = int(np.floor(lo * k * p[j])), int(np.ceil(hi * k * p[j]))
            cats["c%d" % c]["f%d" % j] = {"min": a, "max": b}
            fmin.append(a)
            fmax.append(b)
            fcat.append(c)
        cols.append(base + rng.choice(nf, size=n, p=p))
        base += nf
    pf = np.stack(cols, axis=1).tolist()
    return cats, fmin, fmax, fcat, pf


def _finish(cats, fmin, fmax, fcat, pf, k):
    """(categories, agents, OracleInstance) of a pool given as arrays (feature order = category order)."""
    names = [(c, f) for c in cats for f in cats[c]]
    agents = {i: {names[g][0]: names[g][1] for g in row} for i, row in enumerate(pf)}
    o = OracleInstance(k=k, cat_names=list(cats), feat_names=names, fmin=list(fmin), fmax=list(fmax),
                       fcat=list(fcat), person_feat=pf)
    return cats, agents, o


# ---- the k-th pick's cascade ------------------------------------------------------------------------

def _last_pick_cascades(o, k, seed, begin, S):
    """Pure-Python restatement of legacy_find over panels [begin, begin + S) (legacy.py:124-200,
    analysis.py:141-159, Philox verification stream) on bit masks, recording for every attempt whether
    its k-th pick filled a feature (so delete_all_in_cat ran after the last pick).  Returns (attempts per
    panel, rejections per panel, attempts with such a cascade that were accepted, attempts with one that
    were rejected or ended in its SelectionError)."""
    n, F = o.n, o.F
    fmin, fmax, pf = o.fmin, o.fmax, o.person_feat
    fmask = [0] * F
    for p, row in enumerate(pf):
        for g in row:
            fmask[g] |= 1 << p
    rem0 = [bin(m).count("1") for m in fmask]
    attempts, rejects, casc_ok, casc_bad = [], [], 0, 0
    for i in range(S):
        panel, attempt, rej = begin + i, 0, 0
        while True:
            sel, rem, present = [0] * F, list(rem0), (1 << n) - 1
            failed = last_cascade = False
            for step in range(k):
                best = None
                for f in range(F):
                    need = fmin[f] - sel[f]
                    if need > 0 and rem[f] < need:
                        failed = True
                        break
                    if rem[f] != 0 and fmax[f] != 0:
                        if (need > -100 * rem[f]) if best is None else (need * best[1] > best[0] * rem[f]):
                            best = (need, rem[f], f)
                if failed:
                    break
                assert best is not None or not present
                if best is not None:
                    m = present & fmask[best[2]]
                    for _ in range(legacy_randint(legacy_word(seed, panel, attempt, step), best[1]) - 1):
                        m &= m - 1
                    pick = (m & -m).bit_length() - 1
                    present &= ~(1 << pick)
                    for g in pf[pick]:
                        sel[g] += 1
                        rem[g] -= 1
                    gone = 0
                    for g in pf[pick]:
                        if sel[g] == fmax[g]:
                            gone |= fmask[g]
                    if gone:
                        last_cascade = step == k - 1
                        present &= ~gone
                        rem = [bin(present & m).count("1") for m in fmask]
                    if any(rem[g] == 0 and sel[g] < fmin[g] for g in range(F)):
                        failed = True
                        break
                if step < k - 1 and not present:
                    failed = True
                    break
            attempt += 1
            ok = not failed and all(sel[f] >= fmin[f] for f in range(F))
            if last_cascade:
                casc_ok += ok
                casc_bad += not ok
            if ok:
                break
            rej += not failed
        attempts.append(attempt)
        rejects.append(rej)
    return np.array(attempts, np.uint32), np.array(rejects, np.uint32), casc_ok, casc_bad


def _tight_pool(kind):
    """Small pools with maxima close to k p, so that the last pick often fills a feature, and minima
    at it, so that such attempts are also often under quota.  "lane": F = 20 (the two-lane kernel and
    the wide kernel fit it; about 600 rejections and 280 SelectionErrors in 2000 panels); "solo" and
    "solo_err": F = 12 (the one-lane kernel and the wide kernel; about 290 rejections, and about 150
    SelectionErrors).  Pools, k and seeds were chosen on the CPU with _last_pick_cascades so that the
    oracle alone meets both floors of test_last_pick_cascade."""
    F_per_cat, n, k, seed = {"lane": ((5, 5, 5, 5), 200, 20, 5), "solo": ((4, 4, 4), 120, 16, 5),
                             "solo_err": ((4, 4, 4), 120, 16, 3)}[kind]
    return _finish(*_pool(F_per_cat, n, k, seed, lo=1.0, hi=1.0), k) + (k,)


_LAST_PICK = {}   # pool kind -> the restatement's and the oracle's results, computed once


def _last_pick_reference(kind, S, seed, begin):
    if kind not in _LAST_PICK:
        cats, agents, o, k = _tight_pool(kind)
        att, rej, casc_ok, casc_bad = _last_pick_cascades(o, k, seed, begin, S)
        _LAST_PICK[kind] = (cats, agents, o, k, att, rej, casc_ok, casc_bad)
    return _LAST_PICK[kind]


@pytest.mark.parametrize("kind,group", [("lane", "lane"), ("lane", "wide"), ("solo", "solo"), ("solo_err", "solo"),
                                        ("solo_err", "wide")])
def test_last_pick_cascade(gpu_available, draw_group, kind, group):
    """A sample in which many attempts fill a feature with their k-th pick: at least 20 of them accepted
    (the cascade is skipped) and at least 20 rejected or SelectionError-classified (it runs, for the
    classifier), counted by the pure-Python restatement; picks, attempts and statistics vs the C oracle,
    and the panels once more with the statistics not requested (every last-pick cascade skipped)."""
    P = pkg()
    A = pkg("analysis")
    S, seed, begin = 2000, 17, 123456
    cats, agents, o, k, att, rej, casc_ok, casc_bad = _last_pick_reference(kind, S, seed, begin)
    print("last-pick cascades: accepted %d, rejected or SelectionError %d, attempts %d" % (casc_ok, casc_bad, att.sum()))
    assert casc_ok >= 20 and casc_bad >= 20
    draw_group(group)
    enc = P.encode(cats, agents)
    assert _kernel_name(enc, k).startswith("draw_%s_kernel" % group)
    opanels, oatt, _, orej = _check_against_oracle(enc, o, k, S, seed, begin)
    # the restatement counted the sample the oracle drew
    assert np.array_equal(att, oatt) and np.array_equal(rej, orej)
    A.draw_stats(enc, reset=True)
    assert np.array_equal(_redraw_panels(enc, k, S, seed, begin), opanels)
    assert A.draw_stats(enc) == {"attempts": 0, "rejections": 0, "selection_errors": 0}


# ---- the mirrored second lane -----------------------------------------------------------------------

def _ends_pool(F_per_cat, n, k, seed, lo=0.8, hi=1.25):
    """A random pool plus a leading category "z": z0 held by the LAST agent alone and z1 by the FIRST
    agent alone, both with min = max = 1, z2 by everybody else (min = max = k - 2).  z0 and z1 have the
    largest ratio (1 / 1) at the start, so every attempt picks agent n - 1 first (the second lane's
    very first position) and agent 0 second (the first lane's)."""
    cats, fmin, fmax, fcat, pf = _pool(F_per_cat, n, k, seed, lo, hi)
    zc = {"z": {"z0": {"min": 1, "max": 1}, "z1": {"min": 1, "max": 1}, "z2": {"min": k - 2, "max": k - 2}}}
    zc.update(cats)
    pf = [[2 if 0 < p < n - 1 else (0 if p == n - 1 else 1)] + [g + 3 for g in row] for p, row in enumerate(pf)]
    return _finish(zc, [1, 1, k - 2] + fmin, [1, 1, k - 2] + fmax, [0, 0, 0] + [c + 1 for c in fcat], pf, k)


@pytest.mark.parametrize("F_per_cat,n,k,wn", [
    ((7, 7), 65, 8, 4), ((7, 7), 127, 10, 4), ((5, 5, 5), 128, 10, 4),      # W = 2
    ((5, 5, 5), 129, 10, 4),                                               # W = 3: a padding word in lane 1
    ((8, 8, 8, 5), 64 * 5 - 1, 14, 8), ((7, 7), 64 * 5 - 63, 14, 8),        # W = 5 of 8
    ((6, 6, 6), 64 * 8 - 1, 16, 8), ((6, 6, 6), 64 * 8 - 63, 16, 8),        # W = 8 of 8
    ((7, 7, 7), 64 * 13 - 1, 20, 16), ((7, 7, 7), 64 * 16 - 63, 20, 16),    # W = 13 / 16 of 16
    ((8, 8, 8, 5), 64 * 27 - 1, 24, 28), ((8, 8, 8, 5), 64 * 27 - 63, 24, 28),   # W = 27 of 28 (the sf_e shape)
    ((6, 6, 6), 64 * 28 - 63, 24, 28),                                     # W = 28 of 28
    ((8, 8, 8, 5), 64 * 29 - 63, 24, 32), ((6, 6, 6), 64 * 32 - 1, 24, 32),  # W = 29 / 32 of 32
    ((6, 6, 6), 64 * 32 - 63, 200, 32),                                    # a min above 127: the 16-bit keys
])
def test_mirrored_lane_matches_oracle(gpu_available, F_per_cat, n, k, wn):
    """draw_lane_kernel on two-lane pools (17 <= F <= 32) of odd and even W, with and without padding
    words, whose last word ends at bit 62 (n = 64 W - 1) or bit 0 (n = 64 W - 63): every attempt's first
    holder sought is the very last agent and its second the very first one."""
    P = pkg()
    cats, agents, o = _ends_pool(F_per_cat, n, k, seed=n + k)
    assert 17 <= o.F <= 32
    enc = P.encode(cats, agents)
    name = _kernel_name(enc, k)
    assert name.startswith("draw_lane_kernel<32, %d," % wn), name
    assert name.endswith("true>") == (max(o.fmin) <= 127)
    S = 1500 if k < 100 else 600
    _, _, opicks, _ = _check_against_oracle(enc, o, k, S, seed=k, begin=77000)
    assert np.all(opicks[:, 0] == n - 1) and np.all(opicks[:, 1] == 0)


# ---- the slack bit planes ---------------------------------------------------------------------------

def _slack_pool(kind, slack, seed):
    """A pool whose largest max - selected is exactly ``slack``: feature a0 has min = max = slack (every
    panel fills it, through all of its planes, and cascades), every other maximum is capped at ``slack``.
    "lane": F = 19; "solo": F = 15."""
    k = slack + 8
    n = 640 if slack < 64 else 1280 if slack < 200 else 2040
    rng = np.random.default_rng(seed)
    per_cat = (8, 8) if kind == "lane" else (6, 6)
    cats, fmin, fmax, fcat, pf = _pool(per_cat, n, k, seed, lo=0.8, hi=1.2)
    for c in list(cats):
        for f in cats[c]:
            cats[c][f]["max"] = min(cats[c][f]["max"] + 1, slack)
    fmax = [min(m + 1, slack) for m in fmax]
    ac = {"a": {"a0": {"min": slack, "max": slack}, "a1": {"min": 0, "max": slack}, "a2": {"min": 0, "max": slack}}}
    ac.update(cats)
    col = rng.choice(3, size=n, p=[0.6, 0.2, 0.2])
    pf = [[int(col[p])] + [g + 3 for g in row] for p, row in enumerate(pf)]
    return _finish(ac, [slack, 0, 0] + fmin, [slack] * 3 + fmax, [0, 0, 0] + [c + 1 for c in fcat], pf, k) + (k,)


@pytest.mark.parametrize("kind", ["lane", "solo"])
@pytest.mark.parametrize("slack,planes", [(31, 5), (32, 7), (127, 7), (128, 8), (255, 8), (256, 0)])
def test_slack_plane_counts_match_oracle(gpu_available, kind, slack, planes):
    """The register kernels' plane counts (5, 7, 8) at their edges: the largest max - selected equal to
    2^P - 1 (the last instance that fits P planes) and 2^P (the first that needs more; 256 leaves the
    register kernels), in both kernels, with a feature that counts its whole slack down to the cascade."""
    P = pkg()
    cats, agents, o, k = _slack_pool(kind, slack, seed=slack)
    assert max(o.fmax) == slack
    enc = P.encode(cats, agents)
    name = _kernel_name(enc, k)
    if planes:
        assert name.startswith("draw_%s_kernel<" % kind) and name.split(", ")[-2] == str(planes), name
        assert name.endswith("true>") == (slack <= 127)
    else:
        assert name.startswith("draw_wide_kernel"), name
    _, _, opicks, _ = _check_against_oracle(enc, o, k, 1000 if slack < 200 else 500, seed=9, begin=31000)
    a0 = np.array([row[0] == 0 for row in o.person_feat])
    assert np.all(a0[opicks].sum(axis=1) == slack)
